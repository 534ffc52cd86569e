// hg_lanes.cpp — the service lanes (hg_lane_*, include/handel_gpu.h): batches in
// flight beside each other on their own streams and workspaces, each through
// the body of an aggregate submission (aggregate_device_locked, hg_aggregate.h)
// at the table level the context has built. State: hg_lane in hg_ctx.h.
#include "hg_aggregate.h"

// a lane's largest batch: n requests over max_words bitset words
static FoldCaps fold_caps_lane(size_t n, size_t max_words) {
  const size_t terms = 8 * (max_words + n) + n;  // sum of fold_terms_bound over the batch
  return FoldCaps{terms, terms / (size_t)gt_chunk() + n};
}

extern "C" {

int hg_lane_create(hg_ctx* c, size_t max_batch, size_t max_words, int overlap, hg_lane** out) {
  if (!c || !out || max_batch == 0 || max_batch > (size_t)INT32_MAX || max_words > ((size_t)1 << 40))
    return HG_ERR_ARG;
  *out = nullptr;
  std::lock_guard<std::mutex> g(c->mu);
  HG_CHECK(c, hipSetDevice(c->device));
  hg_lane* l = new hg_lane();
  l->c = c;
  l->pol.overlap = overlap != 0;
  l->max_batch = max_batch;
  l->max_words = max_words;
  // staging: requests | signatures | words, each 256-byte aligned
  const size_t bytes = ((max_batch * sizeof(hg_request) + 255) & ~(size_t)255) +
                       ((max_batch * 64 + 255) & ~(size_t)255) + max_words * 8 + 256;
  hipError_t e = l->s.create(hipStreamNonBlocking);
  if (e == hipSuccess) e = l->done.create(hipEventDisableTiming);
  if (e == hipSuccess) e = l->ev_in.create(hipEventDisableTiming);
  if (e == hipSuccess) e = l->h_in.alloc(bytes);
  if (e == hipSuccess) e = l->h_codes.alloc(max_batch);
  if (e == hipSuccess) e = l->d_in.ensure(bytes);
  if (e == hipSuccess) e = l->d_codes.ensure(max_batch);
  // every workspace at its largest now (ws_ensure)
  if (e == hipSuccess)
    e = ws_ensure(l->ws, max_batch,
                  kWsVerify | kWsLevel | kWsG2Fold | kWsGtFold | kWsPairing | (l->pol.overlap ? kWsSide : 0),
                  fold_caps_lane(max_batch, max_words),
                  sig_form_ws_bytes(sig_form(sig_env(), l->pol, max_batch), (int)max_batch));
  if (e != hipSuccess) {
    c->err = std::string("hg_lane_create: ") + hipGetErrorString(e);
    delete l;
    return HG_ERR_DEVICE;
  }
  c->lanes.push_back(l);
  *out = l;
  return HG_OK;
}

void hg_lane_destroy(hg_lane* l) {
  if (!l) return;
  hg_ctx* c = l->c;
  std::lock_guard<std::mutex> g(c->mu);
  (void)hipSetDevice(c->device);
  (void)hipStreamSynchronize(l->s);
  if (l->ws.side) (void)hipStreamSynchronize(l->ws.side);
  for (size_t i = 0; i < c->lanes.size(); i++)
    if (c->lanes[i] == l) {
      c->lanes.erase(c->lanes.begin() + (long)i);
      break;
    }
  delete l;
}

int hg_lane_stage(hg_lane* l, size_t n, size_t nwords, hg_request** reqs, uint8_t** sigs, uint64_t** words) {
  if (!l || !reqs || !sigs || !words || n == 0 || n > l->max_batch || nwords > l->max_words) return HG_ERR_ARG;
  l->n = n;
  l->nwords = nwords;
  l->off_sigs = (n * sizeof(hg_request) + 255) & ~(size_t)255;
  l->off_words = (l->off_sigs + n * 64 + 255) & ~(size_t)255;
  l->in_bytes = l->off_words + nwords * 8;
  *reqs = reinterpret_cast<hg_request*>(l->h_in.get());
  *sigs = l->h_in.get() + l->off_sigs;
  *words = reinterpret_cast<uint64_t*>(l->h_in.get() + l->off_words);
  return HG_OK;
}

int hg_lane_submit(hg_lane* l) {
  if (!l || l->n == 0) return HG_ERR_ARG;
  hg_ctx* c = l->c;
  const size_t n = l->n;
  const hg_request* h_reqs = reinterpret_cast<const hg_request*>(l->h_in.get());
  // exact fold capacities from the requests, and no bitset read outside the
  // staged words: of any request, level errors included (the host entry points
  // let those pass, hg_requests.h). c->nreg is read only once the lock is held,
  // and this rule does not depend on it.
  FoldCaps caps;
  const auto add = [&caps](const hg_request& r) { caps.add(r.bitlen); };
  if (first_request_outside(h_reqs, n, 0, l->nwords, WordsRule::kEveryRequest, nullptr, add) != kNoRequest)
    return HG_ERR_ARG;
  std::lock_guard<std::mutex> g(c->mu);
  HG_CHECK(c, hipSetDevice(c->device));
  // after the context's last submission (a registry load, a hash, a table
  // build); the lanes' own batches are independent of each other
  if (c->last_ev) HG_CHECK(c, hipStreamWaitEvent(l->s, c->last_ev, 0));
  uint8_t* d = l->d_in.p;
  HG_CHECK(c, hipMemcpyAsync(d, l->h_in.get(), l->in_bytes, hipMemcpyHostToDevice, l->s));
  const AggBatch b{reinterpret_cast<const hg_request*>(d), n, reinterpret_cast<const uint64_t*>(d + l->off_words),
                   d + l->off_sigs, l->d_codes.p, nullptr, nullptr, nullptr, &caps};
  int rc = aggregate_device_locked(c, b, true, l->s, l->ws, l->pol, true);
  if (rc) return rc;
  HG_CHECK(c, hipMemcpyAsync(l->h_codes.get(), l->d_codes.p, n * sizeof(int32_t), hipMemcpyDeviceToHost, l->s));
  HG_CHECK(c, hipEventRecord(l->done, l->s));
  l->recorded = true;
  (void)hipStreamQuery(l->s);  // flush: start now
  return HG_OK;
}

void* hg_lane_stream(hg_lane* l) { return l ? (void*)l->s.h : nullptr; }

int hg_lane_set_pairing_padding(hg_lane* l, int pad) {
  if (!l) return HG_ERR_ARG;
  hg_ctx* c = l->c;
  std::lock_guard<std::mutex> g(c->mu);
  // the lane's pairing workspace at its largest batch now (never grown between
  // batches): the unpadded lane runs the 12-lane form on evaluated lines
  SigPolicy pol = l->pol;
  pol.pad = pad != 0;
  if (const size_t bytes = sig_form_ws_bytes(sig_form(sig_env(), pol, l->max_batch), (int)l->max_batch)) {
    HG_CHECK(c, hipSetDevice(c->device));
    HG_CHECK(c, hipStreamSynchronize(l->s));
    if (l->ws.side) HG_CHECK(c, hipStreamSynchronize(l->ws.side));
    HG_CHECK(c, l->ws.sig_lines.ensure(bytes));
  }
  l->pol = pol;
  return HG_OK;
}

int hg_lane_set_latency_form(hg_lane* l, int max_checks) {
  if (!l || max_checks < 0) return HG_ERR_ARG;
  std::lock_guard<std::mutex> g(l->c->mu);
  l->pol.w2_max = max_checks < kSigW2MaxN ? max_checks : kSigW2MaxN;
  return HG_OK;
}

int hg_lane_submit_device(hg_lane* l, const hg_request* d_reqs, size_t n, const uint64_t* d_words,
                          const uint8_t* d_sigs, int32_t* d_codes, uint8_t* d_bits, void* stream) {
  if (!l || !d_reqs || !d_sigs || !d_codes || n == 0 || n > l->max_batch) return HG_ERR_ARG;
  hg_ctx* c = l->c;
  std::lock_guard<std::mutex> g(c->mu);
  HG_CHECK(c, hipSetDevice(c->device));
  hipStream_t caller = stream ? (hipStream_t)stream : c->stream;
  // after the caller's earlier work on `stream` (its inputs, its last reads of
  // d_codes / d_bits) and the context's last submission
  HG_CHECK(c, hipEventRecord(l->ev_in, caller));
  HG_CHECK(c, hipStreamWaitEvent(l->s, l->ev_in, 0));
  if (c->last_ev) HG_CHECK(c, hipStreamWaitEvent(l->s, c->last_ev, 0));
  const FoldCaps caps = fold_caps_worst(c, n);  // the device words are not visible to the host
  const AggBatch b{d_reqs, n, d_words, d_sigs, d_codes, nullptr, nullptr, d_bits, &caps};
  int rc = aggregate_device_locked(c, b, true, l->s, l->ws, l->pol, true);
  if (rc) return rc;
  HG_CHECK(c, hipEventRecord(l->done, l->s));
  l->recorded = true;
  HG_CHECK(c, hipStreamWaitEvent(caller, l->done, 0));  // the verdicts, in the caller's stream order
  return HG_OK;
}

int hg_lane_query(hg_lane* l) {
  if (!l) return -HG_ERR_ARG;
  if (!l->recorded) return 1;
  hipError_t e = hipEventQuery(l->done);
  if (e == hipSuccess) return 1;
  if (e == hipErrorNotReady) return 0;
  return -HG_ERR_DEVICE;
}

int hg_lane_wait(hg_lane* l) {
  if (!l) return HG_ERR_ARG;
  if (!l->recorded) return HG_OK;
  return hipEventSynchronize(l->done) == hipSuccess ? HG_OK : HG_ERR_DEVICE;
}

const int32_t* hg_lane_codes(hg_lane* l) { return l ? l->h_codes.get() : nullptr; }

}  // extern "C"
