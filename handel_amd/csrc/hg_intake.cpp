// hg_intake.cpp — packet intake and the device-resident stores behind
// include/handel_gpu.h: hg_parse_packets* (hg_packets.hip) and every
// hg_stores_* call (hg_stores.hip, hg_merge.hip). The context, the submission
// chain and the store set's state are in hg_ctx.h.
#include <cstdio>

#include "hg_ctx.h"

extern "C" {

// ---------------------------------------------------------------- packet intake
static bool packet_args_ok(const hg_ctx* c, size_t n, size_t stride) {
  // slot word offsets (2n slots of `stride` words) are 32-bit
  return n <= (size_t)INT32_MAX / 2 && stride >= pkt_stride_words(c->nreg) && stride <= (size_t)INT32_MAX &&
         (n == 0 || 2 * n <= (size_t)UINT32_MAX / stride);
}

size_t hg_packet_stride_words(hg_ctx* c) {
  if (!c) return 0;
  std::lock_guard<std::mutex> g(c->mu);
  return pkt_stride_words(c->nreg);
}

int hg_parse_packets_device(hg_ctx* c, const uint8_t* d_pool, size_t pool_len, const hg_packet* d_pkts, size_t n,
                            size_t stride_words, hg_request* d_reqs, uint64_t* d_words, uint8_t* d_sigs,
                            int32_t* d_codes, void* stream) {
  if (!c || (n && (!d_pkts || !d_reqs || !d_words || !d_sigs || !d_codes)) || (pool_len && !d_pool)) return HG_ERR_ARG;
  if (n == 0) return HG_OK;
  std::lock_guard<std::mutex> g(c->mu);
  if (!packet_args_ok(c, n, stride_words)) return HG_ERR_ARG;
  HG_CHECK(c, hipSetDevice(c->device));
  hipStream_t s = stream ? (hipStream_t)stream : c->stream;
  Submission sub(c, s);
  HG_CHECK(c, sub.start());
  launch_parse_packets(d_pool, pool_len, d_pkts, (int)n, (uint32_t)c->nreg, c->flavor, (int)stride_words, d_reqs,
                       d_words, d_sigs, d_codes, s);
  int rc = check_launch(c);
  if (rc) return rc;
  HG_CHECK(c, sub.finish());
  return HG_OK;
}

int hg_parse_packets(hg_ctx* c, const uint8_t* pool, size_t pool_len, const hg_packet* pkts, size_t n,
                     size_t stride_words, hg_request* reqs, uint64_t* words, uint8_t* sigs, int32_t* codes) {
  if (!c || (n && (!pkts || !reqs || !words || !sigs || !codes)) || (pool_len && !pool)) return HG_ERR_ARG;
  if (n == 0) return HG_OK;
  for (size_t i = 0; i < n; i++) {
    const hg_packet& p = pkts[i];
    if ((uint64_t)p.ms_off + p.ms_len > pool_len ||
        ((p.flags & HG_PKT_HAS_IND) && (uint64_t)p.ind_off + p.ind_len > pool_len))
      return HG_ERR_ARG;
  }
  std::lock_guard<std::mutex> g(c->mu);
  if (!packet_args_ok(c, n, stride_words)) return HG_ERR_ARG;
  HG_CHECK(c, hipSetDevice(c->device));
  const size_t nw = 2 * n * stride_words;
  HG_CHECK(c, c->bytes_a.ensure(pool_len ? pool_len : 1));
  HG_CHECK(c, c->bytes_b.ensure(2 * n * 64));
  HG_CHECK(c, c->pkts.ensure(n));
  HG_CHECK(c, c->reqs.ensure(2 * n));
  HG_CHECK(c, c->words.ensure(nw));
  HG_CHECK(c, c->codes_a.ensure(2 * n));
  Submission sub(c, c->stream);
  HG_CHECK(c, sub.start());
  if (pool_len) HG_CHECK(c, hipMemcpyAsync(c->bytes_a.p, pool, pool_len, hipMemcpyHostToDevice, c->stream));
  HG_CHECK(c, hipMemcpyAsync(c->pkts.p, pkts, n * sizeof(hg_packet), hipMemcpyHostToDevice, c->stream));
  launch_parse_packets(c->bytes_a.p, pool_len, c->pkts.p, (int)n, (uint32_t)c->nreg, c->flavor, (int)stride_words,
                       c->reqs.p, c->words.p, c->bytes_b.p, c->codes_a.p, c->stream);
  int rc = check_launch(c);
  if (rc) return rc;
  HG_CHECK(c, hipMemcpyAsync(reqs, c->reqs.p, 2 * n * sizeof(hg_request), hipMemcpyDeviceToHost, c->stream));
  HG_CHECK(c, hipMemcpyAsync(words, c->words.p, nw * sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
  HG_CHECK(c, hipMemcpyAsync(sigs, c->bytes_b.p, 2 * n * 64, hipMemcpyDeviceToHost, c->stream));
  HG_CHECK(c, hipMemcpyAsync(codes, c->codes_a.p, 2 * n * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
  HG_CHECK(c, sub.finish());
  HG_CHECK(c, hipStreamSynchronize(c->stream));
  return HG_OK;
}

int hg_packet_error(hg_ctx* c, int code, const hg_packet* p, char* buf, size_t cap) {
  if (!c || !p || (cap && !buf)) return -1;
  size_t nreg;
  int flavor;
  {
    std::lock_guard<std::mutex> g(c->mu);
    nreg = c->nreg;
    flavor = c->flavor;
  }
  if (code == HG_ERR_PKT_LEVEL) return snprintf(buf, cap, "invalid packet's level %d", (int)p->level);
  if (code == HG_ERR_PKT_ID_RANGE) {
    // partitioner.go:113-115 (the receiver's range at the packet's level)
    uint32_t lo = 0, hi = 0;
    (void)pkt_range_level(p->receiver, (uint32_t)nreg, (int)p->level, lo, hi);
    return snprintf(buf, cap, "globalID outside level's range. id=%d, min=%u, max=%u, level=%d", (int)p->origin, lo,
                    hi, (int)p->level);
  }
  return snprintf(buf, cap, "%s", hg_code_string(code, flavor));
}

// ---------------------------------------------------------------- stores
// true while the store set's registry is the context's (call with c->mu held)
static bool stores_current(const hg_stores* st) {
  return st->reg_gen == st->c->reg_gen && st->nreg == st->c->nreg && st->nreg > 0;
}

int hg_stores_create(hg_ctx* c, const uint32_t* receivers, size_t n_receivers, size_t max_packets, hg_stores** out) {
  if (out) *out = nullptr;
  if (!c || !receivers || !out || n_receivers == 0 || max_packets == 0 || max_packets > kStoreMaxPackets)
    return HG_ERR_ARG;
  std::lock_guard<std::mutex> g(c->mu);
  const size_t nreg = c->nreg;
  const int levels = pkt_log2_ceil(nreg);
  if (nreg == 0 || levels < 1 || levels > kStoreMaxLevels || n_receivers > nreg) return HG_ERR_ARG;
  std::vector<int32_t> map(nreg, -1);
  for (size_t i = 0; i < n_receivers; i++) {
    if (receivers[i] >= nreg || map[receivers[i]] >= 0) return HG_ERR_ARG;
    map[receivers[i]] = (int32_t)i;
  }
  HG_CHECK(c, hipSetDevice(c->device));
  hg_stores* st = new hg_stores();
  st->c = c;
  st->reg_gen = c->reg_gen;
  st->nreg = nreg;
  st->max_packets = max_packets;
  st->levels = levels;
  st->stride = (int)pkt_stride_words(nreg);
  st->receivers.assign(receivers, receivers + n_receivers);
  st->map = std::move(map);
  const size_t rows = n_receivers * (size_t)levels;
  const size_t n2 = 2 * max_packets;
  size_t temp_bytes = 0;
  hipError_t e = store_select_temp_bytes(n2, n_receivers, &temp_bytes);
  if (e == hipSuccess) e = st->tab.ensure(2 * rows * st->stride);
  if (e == hipSuccess) e = st->flags.ensure(rows);
  if (e == hipSuccess) e = st->d_map.ensure(nreg);
  if (e == hipSuccess) e = st->keys_a.ensure(n2);
  if (e == hipSuccess) e = st->keys_b.ensure(n2);
  if (e == hipSuccess) e = st->cnt.ensure(n_receivers + 1);
  if (e == hipSuccess) e = st->picks.ensure(n_receivers + 1);
  if (e == hipSuccess) e = st->base.ensure(n_receivers + 1);
  if (e == hipSuccess) e = st->temp.ensure(temp_bytes ? temp_bytes : 1);
  Submission sub(c, c->stream);
  if (e == hipSuccess) e = sub.start();
  if (e == hipSuccess) e = hipMemsetAsync(st->tab.p, 0, st->tab.cap * sizeof(uint64_t), c->stream);
  if (e == hipSuccess) e = hipMemsetAsync(st->flags.p, 0, st->flags.cap * sizeof(uint32_t), c->stream);
  if (e == hipSuccess)
    e = hipMemcpyAsync(st->d_map.p, st->map.data(), nreg * sizeof(int32_t), hipMemcpyHostToDevice, c->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  if (e != hipSuccess) {
    c->err = std::string("hg_stores_create: ") + hipGetErrorString(e);
    delete st;
    return HG_ERR_DEVICE;
  }
  *out = st;
  return HG_OK;
}

void hg_stores_destroy(hg_stores* st) {
  if (!st) return;
  hg_ctx* c = st->c;
  std::lock_guard<std::mutex> g(c->mu);
  (void)hipSetDevice(c->device);
  (void)hipStreamSynchronize(c->stream);
  if (c->last_ev) (void)hipEventSynchronize(c->last_ev);  // a submission on a caller stream
  delete st;  // frees its buffers: under the lock, after the sync
}

int hg_stores_update(hg_stores* st, const hg_store_update* ups, size_t n, const uint64_t* words, size_t nwords) {
  if (!st || (n && !ups) || (nwords && !words)) return HG_ERR_ARG;
  hg_ctx* c = st->c;
  std::lock_guard<std::mutex> g(c->mu);
  if (!stores_current(st)) return HG_ERR_ARG;
  if (n == 0) return HG_OK;
  if (n > st->receivers.size() * (size_t)st->levels) return HG_ERR_ARG;  // each (receiver, level) at most once
  std::vector<bool> seen(st->receivers.size() * (size_t)st->levels, false);
  for (size_t i = 0; i < n; i++) {
    const hg_store_update& u = ups[i];
    uint32_t lo = 0, hi = 0;
    if (u.receiver >= st->nreg || st->map[u.receiver] < 0 || u.level < 1 || u.level > (uint32_t)st->levels ||
        !pkt_range_level(u.receiver, (uint32_t)st->nreg, (int)u.level, lo, hi))
      return HG_ERR_ARG;
    const size_t nw = ((size_t)(hi - lo) + 63) / 64;
    if ((uint64_t)u.indiv_off + nw > nwords || ((u.flags & HG_STORE_HAS_BEST) && (uint64_t)u.best_off + nw > nwords))
      return HG_ERR_ARG;
    const size_t row = (size_t)st->map[u.receiver] * st->levels + (u.level - 1);
    if (seen[row]) return HG_ERR_ARG;
    seen[row] = true;
  }
  HG_CHECK(c, hipSetDevice(c->device));
  HG_CHECK(c, st->ups.ensure(n));
  HG_CHECK(c, st->up_words.ensure(nwords ? nwords : 1));
  Submission sub(c, c->stream);
  HG_CHECK(c, sub.start());
  HG_CHECK(c, hipMemcpyAsync(st->ups.p, ups, n * sizeof(hg_store_update), hipMemcpyHostToDevice, c->stream));
  if (nwords)
    HG_CHECK(c, hipMemcpyAsync(st->up_words.p, words, nwords * sizeof(uint64_t), hipMemcpyHostToDevice, c->stream));
  launch_store_update(st->table(), st->ups.p, (int)n, st->up_words.p, c->stream);
  int rc = check_launch(c);
  if (rc) return rc;
  HG_CHECK(c, sub.finish());
  HG_CHECK(c, hipStreamSynchronize(c->stream));
  return HG_OK;
}

int hg_stores_read(hg_stores* st, uint32_t receiver, uint32_t level, uint64_t* best, uint64_t* indiv, int* has_best) {
  if (!st) return HG_ERR_ARG;
  hg_ctx* c = st->c;
  std::lock_guard<std::mutex> g(c->mu);
  if (!stores_current(st)) return HG_ERR_ARG;
  if (receiver >= st->nreg || st->map[receiver] < 0 || level < 1 || level > (uint32_t)st->levels) return HG_ERR_ARG;
  HG_CHECK(c, hipSetDevice(c->device));
  const size_t row = (size_t)st->map[receiver] * st->levels + (level - 1);
  const uint64_t* src = st->tab.p + 2 * row * st->stride;
  const size_t bytes = (size_t)st->stride * sizeof(uint64_t);
  uint32_t flags = 0;
  Submission sub(c, c->stream);
  HG_CHECK(c, sub.start());
  if (best) HG_CHECK(c, hipMemcpyAsync(best, src, bytes, hipMemcpyDeviceToHost, c->stream));
  if (indiv) HG_CHECK(c, hipMemcpyAsync(indiv, src + st->stride, bytes, hipMemcpyDeviceToHost, c->stream));
  HG_CHECK(c, hipMemcpyAsync(&flags, st->flags.p + row, sizeof(flags), hipMemcpyDeviceToHost, c->stream));
  HG_CHECK(c, sub.finish());
  HG_CHECK(c, hipStreamSynchronize(c->stream));
  if (has_best) *has_best = (flags & HG_STORE_HAS_BEST) ? 1 : 0;
  return HG_OK;
}

// n and the slot stride of an evaluate call against the store set's registry
static bool stores_slots_ok(const hg_stores* st, size_t n, size_t stride) {
  return n <= kStoreMaxPackets && stride >= (size_t)st->stride && stride <= (size_t)INT32_MAX &&
         (n == 0 || 2 * n <= (size_t)UINT32_MAX / stride);
}

// the scores of n checked packets, device pointers, on stream s (no sync)
static int stores_evaluate_locked(hg_stores* st, const hg_packet* d_pkts, size_t n, size_t stride_words,
                                  const uint64_t* d_words, const int32_t* d_codes, const uint8_t* d_live,
                                  int32_t* d_scores, hipStream_t s) {
  hg_ctx* c = st->c;
  Submission sub(c, s);
  HG_CHECK(c, sub.start());
  launch_store_evaluate(st->table(), d_pkts, (int)n, (int)stride_words, d_words, d_codes, d_live, d_scores, s);
  int rc = check_launch(c);
  if (rc) return rc;
  HG_CHECK(c, sub.finish());
  return HG_OK;
}

int hg_stores_evaluate_device(hg_stores* st, const hg_packet* d_pkts, size_t n, size_t stride_words,
                              const uint64_t* d_words, const int32_t* d_codes, const uint8_t* d_live,
                              int32_t* d_scores, void* stream) {
  if (!st || (n && (!d_pkts || !d_words || !d_codes || !d_scores))) return HG_ERR_ARG;
  hg_ctx* c = st->c;
  std::lock_guard<std::mutex> g(c->mu);
  if (!stores_current(st) || !stores_slots_ok(st, n, stride_words)) return HG_ERR_ARG;
  if (n == 0) return HG_OK;
  HG_CHECK(c, hipSetDevice(c->device));
  hipStream_t s = stream ? (hipStream_t)stream : c->stream;
  return stores_evaluate_locked(st, d_pkts, n, stride_words, d_words, d_codes, d_live, d_scores, s);
}

int hg_stores_evaluate(hg_stores* st, const hg_packet* pkts, size_t n, size_t stride_words, const uint64_t* words,
                       const int32_t* codes, const uint8_t* live, int32_t* scores) {
  if (!st || (n && (!pkts || !words || !codes || !scores))) return HG_ERR_ARG;
  hg_ctx* c = st->c;
  std::lock_guard<std::mutex> g(c->mu);
  if (!stores_current(st) || !stores_slots_ok(st, n, stride_words) || n > st->max_packets) return HG_ERR_ARG;
  if (n == 0) return HG_OK;
  HG_CHECK(c, hipSetDevice(c->device));
  const size_t nw = 2 * n * stride_words;
  HG_CHECK(c, st->pkts.ensure(n));
  HG_CHECK(c, st->words.ensure(nw));
  HG_CHECK(c, st->codes.ensure(2 * n));
  HG_CHECK(c, st->scores.ensure(2 * n));
  if (live) HG_CHECK(c, st->live.ensure(2 * n));
  hipStream_t s = c->stream;
  Submission sub(c, s);
  HG_CHECK(c, sub.start());
  HG_CHECK(c, hipMemcpyAsync(st->pkts.p, pkts, n * sizeof(hg_packet), hipMemcpyHostToDevice, s));
  HG_CHECK(c, hipMemcpyAsync(st->words.p, words, nw * sizeof(uint64_t), hipMemcpyHostToDevice, s));
  HG_CHECK(c, hipMemcpyAsync(st->codes.p, codes, 2 * n * sizeof(int32_t), hipMemcpyHostToDevice, s));
  if (live) HG_CHECK(c, hipMemcpyAsync(st->live.p, live, 2 * n, hipMemcpyHostToDevice, s));
  int rc = stores_evaluate_locked(st, st->pkts.p, n, stride_words, st->words.p, st->codes.p,
                                  live ? st->live.p : nullptr, st->scores.p, s);
  if (rc) return rc;
  HG_CHECK(c, hipMemcpyAsync(scores, st->scores.p, 2 * n * sizeof(int32_t), hipMemcpyDeviceToHost, s));
  HG_CHECK(c, sub.finish());
  HG_CHECK(c, hipStreamSynchronize(s));
  return HG_OK;
}

size_t hg_stores_select_capacity(hg_stores* st, size_t n, uint32_t k) {
  if (!st) return 0;
  const size_t S = st->receivers.size();  // fixed at creation
  const size_t n2 = 2 * n;
  return k == 0 ? 0 : (n2 / k < S ? n2 : S * (size_t)k);
}

int hg_stores_select_device(hg_stores* st, const hg_packet* d_pkts, size_t n, const int32_t* d_scores, uint32_t k,
                            const hg_request* d_reqs, const uint8_t* d_sigs, uint32_t* d_sel, uint32_t* d_count,
                            hg_request* d_out_reqs, uint8_t* d_out_sigs, void* stream) {
  if (!st || !d_count || k == 0 || (n && (!d_pkts || !d_scores || !d_reqs || !d_sigs || !d_sel || !d_out_reqs || !d_out_sigs)))
    return HG_ERR_ARG;
  if (((uintptr_t)d_sigs | (uintptr_t)d_out_sigs) & 3) return HG_ERR_ARG;
  hg_ctx* c = st->c;
  std::lock_guard<std::mutex> g(c->mu);
  if (!stores_current(st) || n > st->max_packets) return HG_ERR_ARG;
  HG_CHECK(c, hipSetDevice(c->device));
  if (n) {  // the workspace was sized for max_packets; a smaller batch never needs more
    size_t need = 0;
    HG_CHECK(c, store_select_temp_bytes(2 * n, st->receivers.size(), &need));
    if (need > st->temp.cap) {
      c->err = "hg_stores_select_device: selection workspace too small";
      return HG_ERR_DEVICE;
    }
  }
  hipStream_t s = stream ? (hipStream_t)stream : c->stream;
  Submission sub(c, s);
  HG_CHECK(c, sub.start());
  if (n == 0) {
    HG_CHECK(c, hipMemsetAsync(d_count, 0, sizeof(uint32_t), s));
  } else {
    const StoreSelectWs ws{st->keys_a.p, st->keys_b.p, st->cnt.p, st->picks.p, st->base.p, st->temp.p, st->temp.cap};
    const size_t cap = hg_stores_select_capacity(st, n, k);
    HG_CHECK(c, launch_store_select(st->table(), ws, d_pkts, (int)n, d_scores, k, d_reqs, d_sigs, d_sel, d_count,
                                    d_out_reqs, d_out_sigs, (uint32_t)cap, s));
  }
  HG_CHECK(c, sub.finish());
  return HG_OK;
}

// ---------------------------------------------------------------- stores: merge and Combined
int hg_stores_enable_merge(hg_stores* st) {
  if (!st) return HG_ERR_ARG;
  hg_ctx* c = st->c;
  std::lock_guard<std::mutex> g(c->mu);
  if (!stores_current(st)) return HG_ERR_ARG;
  if (st->merge) return HG_OK;
  HG_CHECK(c, hipSetDevice(c->device));
  const size_t S = st->receivers.size();
  const size_t rows = S * (size_t)st->levels;
  HG_CHECK(c, st->best_sig.ensure(rows * 64));
  HG_CHECK(c, st->indiv_sig.ensure(S * st->nreg * 64));
  HG_CHECK(c, st->held.ensure(rows * st->stride));
  HG_CHECK(c, st->own.ensure(S));
  HG_CHECK(c, st->m_rows.ensure(2 * st->max_packets));
  HG_CHECK(c, st->m_marks.ensure(2 * st->max_packets));
  Submission sub(c, c->stream);
  HG_CHECK(c, sub.start());
  HG_CHECK(c, hipMemsetAsync(st->best_sig.p, 0, st->best_sig.cap, c->stream));
  HG_CHECK(c, hipMemsetAsync(st->indiv_sig.p, 0, st->indiv_sig.cap, c->stream));
  HG_CHECK(c, hipMemsetAsync(st->held.p, 0, st->held.cap * sizeof(uint64_t), c->stream));
  HG_CHECK(c, hipMemsetAsync(st->own.p, 0, st->own.cap * sizeof(uint32_t), c->stream));
  HG_CHECK(c, sub.finish());
  HG_CHECK(c, hipStreamSynchronize(c->stream));
  st->merge = true;
  return HG_OK;
}

int hg_stores_update_sigs(hg_stores* st, const hg_store_sig* recs, size_t n, const uint8_t* sigs, size_t n_sigs) {
  if (!st || (n && (!recs || !sigs))) return HG_ERR_ARG;
  hg_ctx* c = st->c;
  std::lock_guard<std::mutex> g(c->mu);
  if (!stores_current(st) || !st->merge) return HG_ERR_ARG;
  if (n == 0) return HG_OK;
  if (n > (size_t)INT32_MAX) return HG_ERR_ARG;
  for (size_t i = 0; i < n; i++) {
    const hg_store_sig& r = recs[i];
    if (r.receiver >= st->nreg || st->map[r.receiver] < 0 || r.sig_off >= n_sigs) return HG_ERR_ARG;
    if (r.level == 0) continue;
    uint32_t lo = 0, hi = 0;
    if (r.level > (uint32_t)st->levels || !pkt_range_level(r.receiver, (uint32_t)st->nreg, (int)r.level, lo, hi))
      return HG_ERR_ARG;
    if (r.index != HG_STORE_SIG_BEST && r.index >= hi - lo) return HG_ERR_ARG;
  }
  HG_CHECK(c, hipSetDevice(c->device));
  HG_CHECK(c, st->sig_recs.ensure(n));
  HG_CHECK(c, st->sig_bytes.ensure(n_sigs * 64));
  Submission sub(c, c->stream);
  HG_CHECK(c, sub.start());
  HG_CHECK(c, hipMemcpyAsync(st->sig_recs.p, recs, n * sizeof(hg_store_sig), hipMemcpyHostToDevice, c->stream));
  HG_CHECK(c, hipMemcpyAsync(st->sig_bytes.p, sigs, n_sigs * 64, hipMemcpyHostToDevice, c->stream));
  launch_store_update_sigs(st->table(), st->merge_table(), st->sig_recs.p, (int)n, st->sig_bytes.p, c->stream);
  int rc = check_launch(c);
  if (rc) return rc;
  HG_CHECK(c, sub.finish());
  HG_CHECK(c, hipStreamSynchronize(c->stream));
  return HG_OK;
}

int hg_stores_read_best(hg_stores* st, uint32_t receiver, uint32_t level, uint64_t* best, uint8_t* sig, int* flags) {
  if (!st) return HG_ERR_ARG;
  hg_ctx* c = st->c;
  std::lock_guard<std::mutex> g(c->mu);
  if (!stores_current(st) || !st->merge) return HG_ERR_ARG;
  if (receiver >= st->nreg || st->map[receiver] < 0 || level > (uint32_t)st->levels) return HG_ERR_ARG;
  HG_CHECK(c, hipSetDevice(c->device));
  const size_t s = (size_t)st->map[receiver];
  uint32_t fl = 0;
  Submission sub(c, c->stream);
  HG_CHECK(c, sub.start());
  if (level == 0) {
    if (sig)
      HG_CHECK(c, hipMemcpyAsync(sig, st->indiv_sig.p + (s * st->nreg + receiver) * 64, 64, hipMemcpyDeviceToHost,
                                 c->stream));
    HG_CHECK(c, hipMemcpyAsync(&fl, st->own.p + s, sizeof(fl), hipMemcpyDeviceToHost, c->stream));
  } else {
    const size_t row = s * st->levels + (level - 1);
    if (best)
      HG_CHECK(c, hipMemcpyAsync(best, st->tab.p + 2 * row * st->stride, (size_t)st->stride * sizeof(uint64_t),
                                 hipMemcpyDeviceToHost, c->stream));
    if (sig) HG_CHECK(c, hipMemcpyAsync(sig, st->best_sig.p + row * 64, 64, hipMemcpyDeviceToHost, c->stream));
    HG_CHECK(c, hipMemcpyAsync(&fl, st->flags.p + row, sizeof(fl), hipMemcpyDeviceToHost, c->stream));
  }
  HG_CHECK(c, sub.finish());
  HG_CHECK(c, hipStreamSynchronize(c->stream));
  if (level == 0) {
    fl = (fl & 1u) ? (HG_STORE_HAS_BEST | HG_STORE_BEST_SIG) : 0u;
    if (best) {
      for (int w = 0; w < st->stride; w++) best[w] = 0;
      best[0] = fl ? 1u : 0u;
    }
  }
  if (flags) *flags = (int)(fl & (HG_STORE_HAS_BEST | HG_STORE_BEST_SIG));
  return HG_OK;
}

int hg_stores_merge_device(hg_stores* st, const hg_packet* d_pkts, size_t n, const uint32_t* d_sel,
                           const uint32_t* d_count, size_t capacity, const int32_t* d_vcodes, size_t stride_words,
                           const uint64_t* d_words, const uint8_t* d_sigs, int32_t* d_results, uint32_t* d_changed,
                           uint32_t* d_nchanged, void* stream) {
  if (!st || !d_nchanged ||
      (capacity && (!d_pkts || !d_sel || !d_vcodes || !d_words || !d_sigs || !d_results || !d_changed)))
    return HG_ERR_ARG;
  if ((uintptr_t)d_sigs & 3) return HG_ERR_ARG;
  hg_ctx* c = st->c;
  std::lock_guard<std::mutex> g(c->mu);
  if (!stores_current(st) || !st->merge || !stores_slots_ok(st, n, stride_words) || n > st->max_packets ||
      capacity > 2 * st->max_packets)
    return HG_ERR_ARG;
  HG_CHECK(c, hipSetDevice(c->device));
  hipStream_t s = stream ? (hipStream_t)stream : c->stream;
  Submission sub(c, s);
  HG_CHECK(c, sub.start());
  const StoreMergeWs ws{st->m_rows.p, st->m_marks.p};
  launch_store_merge(st->table(), st->merge_table(), ws, d_pkts, (int)n, d_sel, d_count, (uint32_t)capacity, d_vcodes,
                     (int)stride_words, d_words, d_sigs, d_results, d_changed, d_nchanged, s);
  int rc = check_launch(c);
  if (rc) return rc;
  HG_CHECK(c, sub.finish());
  return HG_OK;
}

// m and the row stride of a Combined call against a merging store set
static bool stores_combined_ok(const hg_stores* st, size_t m, size_t words_stride) {
  return stores_current(st) && st->merge && m <= (size_t)INT32_MAX && words_stride != 0 &&
         words_stride <= (size_t)INT32_MAX;
}

// Combined of m queries, device pointers, on stream s (no sync)
static int stores_combined_locked(hg_stores* st, const hg_store_query* d_queries, size_t m, size_t words_stride,
                                  int32_t* d_codes, uint32_t* d_bitlens, uint64_t* d_words, uint8_t* d_sigs,
                                  hipStream_t s) {
  hg_ctx* c = st->c;
  Submission sub(c, s);
  HG_CHECK(c, sub.start());
  launch_store_combined(st->table(), st->merge_table(), d_queries, (int)m, (int)words_stride, d_codes, d_bitlens,
                        d_words, d_sigs, s);
  int rc = check_launch(c);
  if (rc) return rc;
  HG_CHECK(c, sub.finish());
  return HG_OK;
}

int hg_stores_combined_device(hg_stores* st, const hg_store_query* d_queries, size_t m, size_t words_stride,
                              int32_t* d_codes, uint32_t* d_bitlens, uint64_t* d_words, uint8_t* d_sigs,
                              void* stream) {
  if (!st || (m && (!d_queries || !d_codes || !d_bitlens || !d_words || !d_sigs))) return HG_ERR_ARG;
  if ((uintptr_t)d_sigs & 3) return HG_ERR_ARG;
  hg_ctx* c = st->c;
  std::lock_guard<std::mutex> g(c->mu);
  if (!stores_combined_ok(st, m, words_stride)) return HG_ERR_ARG;
  if (m == 0) return HG_OK;
  HG_CHECK(c, hipSetDevice(c->device));
  hipStream_t s = stream ? (hipStream_t)stream : c->stream;
  return stores_combined_locked(st, d_queries, m, words_stride, d_codes, d_bitlens, d_words, d_sigs, s);
}

int hg_stores_combined(hg_stores* st, const hg_store_query* queries, size_t m, size_t words_stride, int32_t* codes,
                       uint32_t* bitlens, uint64_t* words, uint8_t* sigs) {
  if (!st || (m && (!queries || !codes || !bitlens || !words || !sigs))) return HG_ERR_ARG;
  hg_ctx* c = st->c;
  std::lock_guard<std::mutex> g(c->mu);
  if (!stores_combined_ok(st, m, words_stride)) return HG_ERR_ARG;
  if (m == 0) return HG_OK;
  HG_CHECK(c, hipSetDevice(c->device));
  HG_CHECK(c, st->q_in.ensure(m));
  HG_CHECK(c, st->q_codes.ensure(m));
  HG_CHECK(c, st->q_bitlens.ensure(m));
  HG_CHECK(c, st->q_words.ensure(m * words_stride));
  HG_CHECK(c, st->q_sigs.ensure(m * 64));
  hipStream_t s = c->stream;
  Submission sub(c, s);
  HG_CHECK(c, sub.start());
  HG_CHECK(c, hipMemcpyAsync(st->q_in.p, queries, m * sizeof(hg_store_query), hipMemcpyHostToDevice, s));
  int rc = stores_combined_locked(st, st->q_in.p, m, words_stride, st->q_codes.p, st->q_bitlens.p, st->q_words.p,
                                  st->q_sigs.p, s);
  if (rc) return rc;
  HG_CHECK(c, hipMemcpyAsync(codes, st->q_codes.p, m * sizeof(int32_t), hipMemcpyDeviceToHost, s));
  HG_CHECK(c, hipMemcpyAsync(bitlens, st->q_bitlens.p, m * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
  HG_CHECK(c, hipMemcpyAsync(words, st->q_words.p, m * words_stride * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
  HG_CHECK(c, hipMemcpyAsync(sigs, st->q_sigs.p, m * 64, hipMemcpyDeviceToHost, s));
  HG_CHECK(c, sub.finish());
  HG_CHECK(c, hipStreamSynchronize(s));
  return HG_OK;
}

}  // extern "C"
