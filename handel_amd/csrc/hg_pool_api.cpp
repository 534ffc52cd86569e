// hg_pool_api.cpp — the hg_stores_pool_* calls of include/handel_gpu.h: Handel's
// queue of parsed signatures kept in HBM across intake steps (hg_pool.hip).
// A pool belongs to one hg_stores and, like it, to the registry load it was
// created on; every call is a submission of the context (hg_ctx.h).
#include <vector>

#include "hg_ctx.h"
#include "hg_pool.h"

struct hg_pool {
  hg_stores* st = nullptr;
  size_t capacity = 0;
  int cur = 0;       // the side that holds the queue
  size_t bound = 0;  // host-side bound on the occupancy: the last count read back plus every slot offered since
  DevBuf<PoolRec> recs[2];
  DevBuf<uint64_t> words[2];
  DevBuf<uint32_t> sigs[2];
  DevBuf<int32_t> marks[2];
  DevBuf<uint32_t> count;  // one per side
  DevBuf<uint32_t> flags, offs, perm, starts, picks, base;
  DevBuf<uint64_t> keys_a, keys_b;
  DevBuf<uint8_t> temp;
  PoolSide side(int i) const { return PoolSide{recs[i].p, words[i].p, sigs[i].p, marks[i].p, count.p + i}; }
  PoolWs ws() const {
    return PoolWs{flags.p, offs.p, keys_a.p, keys_b.p, perm.p, starts.p, picks.p, base.p, temp.p, temp.cap};
  }
};

// true while the pool's store set belongs to the context's registry (call with c->mu held)
static bool pool_current(const hg_pool* p) {
  const hg_stores* st = p->st;
  return st->reg_gen == st->c->reg_gen && st->nreg == st->c->nreg && st->nreg > 0;
}

// the true count of the queue, read on stream s (one synchronisation); refreshes the bound
static int pool_read_count(hg_pool* p, hipStream_t s, size_t* out) {
  hg_ctx* c = p->st->c;
  uint32_t cnt = 0;
  Submission sub(c, s);
  HG_CHECK(c, sub.start());
  HG_CHECK(c, hipMemcpyAsync(&cnt, p->count.p + p->cur, sizeof(cnt), hipMemcpyDeviceToHost, s));
  HG_CHECK(c, sub.finish());
  HG_CHECK(c, hipStreamSynchronize(s));
  p->bound = cnt < p->capacity ? cnt : p->capacity;
  if (out) *out = p->bound;
  return HG_OK;
}

extern "C" {

int hg_stores_pool_create(hg_stores* st, size_t capacity_slots, hg_pool** out) {
  if (out) *out = nullptr;
  if (!st || !out || capacity_slots == 0 || capacity_slots > 2 * kStoreMaxPackets) return HG_ERR_ARG;
  hg_ctx* c = st->c;
  std::lock_guard<std::mutex> g(c->mu);
  if (!(st->reg_gen == c->reg_gen && st->nreg == c->nreg && st->nreg > 0)) return HG_ERR_ARG;
  HG_CHECK(c, hipSetDevice(c->device));
  hg_pool* p = new hg_pool();
  p->st = st;
  p->capacity = capacity_slots;
  const size_t C = capacity_slots, S = st->receivers.size();
  size_t temp_bytes = 0;
  hipError_t e = pool_temp_bytes(C, S, &temp_bytes);
  for (int i = 0; i < 2 && e == hipSuccess; i++) {
    e = p->recs[i].alloc(C);
    if (e == hipSuccess) e = p->words[i].alloc(C * (size_t)st->stride);
    if (e == hipSuccess) e = p->sigs[i].alloc(C * 16);
    if (e == hipSuccess) e = p->marks[i].alloc(C);
  }
  if (e == hipSuccess) e = p->count.alloc(2);
  if (e == hipSuccess) e = p->flags.alloc(C + 1);
  if (e == hipSuccess) e = p->offs.alloc(C + 1);
  if (e == hipSuccess) e = p->perm.alloc(C);
  if (e == hipSuccess) e = p->keys_a.alloc(C);
  if (e == hipSuccess) e = p->keys_b.alloc(C);
  if (e == hipSuccess) e = p->starts.alloc(S + 1);
  if (e == hipSuccess) e = p->picks.alloc(S + 1);
  if (e == hipSuccess) e = p->base.alloc(S + 1);
  if (e == hipSuccess) e = p->temp.alloc(temp_bytes ? temp_bytes : 1);
  Submission sub(c, c->stream);
  if (e == hipSuccess) e = sub.start();
  if (e == hipSuccess) e = hipMemsetAsync(p->count.p, 0, 2 * sizeof(uint32_t), c->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  if (e != hipSuccess) {
    c->err = std::string("hg_stores_pool_create: ") + hipGetErrorString(e);
    delete p;
    return HG_ERR_DEVICE;
  }
  *out = p;
  return HG_OK;
}

void hg_stores_pool_destroy(hg_pool* p) {
  if (!p) return;
  hg_ctx* c = p->st->c;
  std::lock_guard<std::mutex> g(c->mu);
  (void)hipSetDevice(c->device);
  (void)hipStreamSynchronize(c->stream);
  if (c->last_ev) (void)hipEventSynchronize(c->last_ev);  // a submission on a caller stream
  delete p;
}

size_t hg_stores_pool_bytes(hg_pool* p) {
  if (!p) return 0;
  std::lock_guard<std::mutex> g(p->st->c->mu);
  size_t b = p->count.bytes() + p->flags.bytes() + p->offs.bytes() + p->perm.bytes() + p->starts.bytes() +
             p->picks.bytes() + p->base.bytes() + p->keys_a.bytes() + p->keys_b.bytes() + p->temp.bytes();
  for (int i = 0; i < 2; i++) b += p->recs[i].bytes() + p->words[i].bytes() + p->sigs[i].bytes() + p->marks[i].bytes();
  return b;
}

size_t hg_stores_pool_select_capacity(hg_pool* p, uint32_t k) {
  if (!p || k == 0) return 0;
  const size_t S = p->st->receivers.size();  // fixed at creation
  return p->capacity / k < S ? p->capacity : S * (size_t)k;
}

int hg_stores_pool_append_device(hg_pool* p, const hg_packet* d_pkts, size_t n, size_t stride_words,
                                 const hg_request* d_reqs, const uint64_t* d_words, const uint8_t* d_sigs,
                                 const int32_t* d_codes, const uint8_t* d_live, void* stream) {
  if (!p || (n && (!d_pkts || !d_reqs || !d_words || !d_sigs || !d_codes))) return HG_ERR_ARG;
  if ((uintptr_t)d_sigs & 3) return HG_ERR_ARG;
  hg_stores* st = p->st;
  hg_ctx* c = st->c;
  std::lock_guard<std::mutex> g(c->mu);
  if (!pool_current(p)) return HG_ERR_ARG;
  if (n > kStoreMaxPackets || stride_words < (size_t)st->stride || stride_words > (size_t)INT32_MAX ||
      (n && 2 * n > (size_t)UINT32_MAX / stride_words))
    return HG_ERR_ARG;
  if (n == 0) return HG_OK;
  if (2 * n > p->capacity) return HG_ERR_ARG;
  HG_CHECK(c, hipSetDevice(c->device));
  hipStream_t s = stream ? (hipStream_t)stream : c->stream;
  if (p->bound + 2 * n > p->capacity) {
    int rc = pool_read_count(p, s, nullptr);
    if (rc) return rc;
    if (p->bound + 2 * n > p->capacity) return HG_ERR_ARG;
  }
  Submission sub(c, s);
  HG_CHECK(c, sub.start());
  HG_CHECK(c, launch_pool_append(st->table(), p->side(p->cur), p->ws(), (uint32_t)p->capacity, d_pkts, (int)n,
                                 (int)stride_words, d_reqs, d_words, (const uint32_t*)d_sigs, d_codes, d_live, s));
  p->bound += 2 * n;
  HG_CHECK(c, sub.finish());
  return HG_OK;
}

int hg_stores_pool_step_device(hg_pool* p, uint32_t k, size_t capacity, hg_packet* d_out_pkts, uint32_t* d_sel,
                               uint32_t* d_count, hg_request* d_out_reqs, uint64_t* d_out_words, uint8_t* d_out_sigs,
                               int32_t* d_out_scores, void* stream) {
  if (!p || k == 0 || k > 64 || !d_out_pkts || !d_sel || !d_count || !d_out_reqs || !d_out_words || !d_out_sigs ||
      !d_out_scores)
    return HG_ERR_ARG;
  if ((uintptr_t)d_out_sigs & 3) return HG_ERR_ARG;
  hg_stores* st = p->st;
  hg_ctx* c = st->c;
  std::lock_guard<std::mutex> g(c->mu);
  if (!pool_current(p)) return HG_ERR_ARG;
  if (capacity != hg_stores_pool_select_capacity(p, k) || capacity > st->max_packets ||
      2 * capacity > (size_t)UINT32_MAX / (size_t)st->stride)
    return HG_ERR_ARG;
  HG_CHECK(c, hipSetDevice(c->device));
  hipStream_t s = stream ? (hipStream_t)stream : c->stream;
  Submission sub(c, s);
  HG_CHECK(c, sub.start());
  HG_CHECK(c, launch_pool_step(st->table(), p->side(p->cur), p->side(p->cur ^ 1), p->ws(), (uint32_t)p->capacity, k,
                               (uint32_t)capacity, d_out_pkts, d_sel, d_count, d_out_reqs, d_out_words,
                               (uint32_t*)d_out_sigs, d_out_scores, s));
  p->cur ^= 1;  // the survivors are the queue now
  HG_CHECK(c, sub.finish());
  return HG_OK;
}

int hg_stores_pool_count(hg_pool* p, size_t* count) {
  if (!p || !count) return HG_ERR_ARG;
  hg_ctx* c = p->st->c;
  std::lock_guard<std::mutex> g(c->mu);
  if (!pool_current(p)) return HG_ERR_ARG;
  HG_CHECK(c, hipSetDevice(c->device));
  return pool_read_count(p, c->stream, count);
}

int hg_stores_pool_read(hg_pool* p, uint32_t receiver, size_t cap, hg_packet* pkts, uint8_t* individual,
                        int32_t* scores, size_t* count) {
  if (!p || !count) return HG_ERR_ARG;
  hg_stores* st = p->st;
  hg_ctx* c = st->c;
  std::lock_guard<std::mutex> g(c->mu);
  if (!pool_current(p) || receiver >= st->nreg || st->map[receiver] < 0) return HG_ERR_ARG;
  HG_CHECK(c, hipSetDevice(c->device));
  size_t have = 0;
  int rc = pool_read_count(p, c->stream, &have);
  if (rc) return rc;
  std::vector<PoolRec> recs(have);
  std::vector<int32_t> marks(have);
  if (have) {
    Submission sub(c, c->stream);
    HG_CHECK(c, sub.start());
    HG_CHECK(c, hipMemcpyAsync(recs.data(), p->recs[p->cur].p, have * sizeof(PoolRec), hipMemcpyDeviceToHost,
                               c->stream));
    HG_CHECK(c, hipMemcpyAsync(marks.data(), p->marks[p->cur].p, have * sizeof(int32_t), hipMemcpyDeviceToHost,
                               c->stream));
    HG_CHECK(c, sub.finish());
    HG_CHECK(c, hipStreamSynchronize(c->stream));
  }
  size_t m = 0;
  for (size_t i = 0; i < have; i++) {  // a receiver's slots lie in its queue's order
    const PoolRec& r = recs[i];
    if (r.receiver != receiver) continue;
    if (m < cap) {
      if (pkts) pkts[m] = hg_packet{r.origin, r.receiver, r.level, r.flags, 0u, 0u, 0u, 0u};
      if (individual) individual[m] = r.individual ? 1 : 0;
      if (scores) scores[m] = marks[i];
    }
    m++;
  }
  *count = m;
  return HG_OK;
}

int hg_stores_pool_clear(hg_pool* p) {
  if (!p) return HG_ERR_ARG;
  hg_ctx* c = p->st->c;
  std::lock_guard<std::mutex> g(c->mu);
  if (!pool_current(p)) return HG_ERR_ARG;
  HG_CHECK(c, hipSetDevice(c->device));
  Submission sub(c, c->stream);
  HG_CHECK(c, sub.start());
  HG_CHECK(c, hipMemsetAsync(p->count.p, 0, 2 * sizeof(uint32_t), c->stream));
  HG_CHECK(c, sub.finish());
  HG_CHECK(c, hipStreamSynchronize(c->stream));
  p->bound = 0;
  return HG_OK;
}

}  // extern "C"
