// hg_aggregate.cpp — aggregate verification (processing.go verifySignature)
// behind include/handel_gpu.h: a batch's workspaces and table level, the
// Combine fold and pairing check in their flows (aggregate_device_locked), the
// staging of a batch given by host pointers, and the aggregate and
// multisignature entry points. The GT tables are hg_gttables.cpp's, the service
// lanes hg_lanes.cpp's; what the three share is hg_aggregate.h, the state hg_ctx.h.
#include <cstdio>
#include <cstring>

#include "hg_aggregate.h"

// GT fold workspaces. A request of b bits has at most 8 nonzero 8-bit (4
// 16-bit) windows per registry-aligned 64-bit word of its range, plus the
// block term of a complemented fold.
// Fold schedule: terms per chunk and k_gt_chunks workgroups (HG_GT_CHUNK /
// HG_GT_GRID override them for tuning runs).
int gt_chunk() {
  static const int chunk = env_int("HG_GT_CHUNK", kGtChunk, 1, 64);
  return chunk;
}
static size_t fold_terms_bound(size_t bitlen) { return 8 * ((bitlen + 7 + 63) / 64) + 1; }
void FoldCaps::add(size_t bitlen) {
  const size_t m = fold_terms_bound(bitlen);
  terms += m;
  chunks += (m + gt_chunk() - 1) / gt_chunk();
}
FoldCaps fold_caps_worst(const hg_ctx* c, size_t n) {
  FoldCaps one;
  one.add(c->nreg);
  return FoldCaps{one.terms * n, one.chunks * n};
}

hipError_t ws_ensure(Ws& ws, size_t n, unsigned parts, const FoldCaps& caps, size_t sig_bytes) {
  hipError_t e = hipSuccess;
  auto grow = [&e](auto& buf, size_t count) {
    if (e == hipSuccess) e = buf.ensure(count);
  };
  if (parts & kWsVerify) grow(ws.pts1, n), grow(ws.codes_b, n);
  if (parts & kWsLevel) grow(ws.codes_c, n);
  if (parts & kWsG2Fold) grow(ws.checks, n), grow(ws.order, n), grow(ws.agg_ws, n * agg_partial_bytes() + agg_fixed_bytes());
  if (parts & kWsAggOut) grow(ws.pts2, n);
  if (parts & kWsGtFold) {
    grow(ws.gt_plan, n), grow(ws.gt_hdr, 1), grow(ws.gt_terms, caps.terms), grow(ws.gt_ord, caps.chunks);
    grow(ws.gt_multi, 2 * n), grow(ws.gt_partial, caps.chunks), grow(ws.gt_y, n);
  }
  if (parts & kWsPairing) grow(ws.gt_fe, n), grow(ws.sig_lines, sig_bytes);
  if ((parts & kWsSide) && e == hipSuccess) e = ensure_side(ws);
  return e;
}

static int ensure_gt_fold(hg_ctx* c, Ws& ws, size_t n, const FoldCaps& caps, GtWork& w) {
  static const int grid = env_int("HG_GT_GRID", 4096, 64, 65536);
  if (caps.chunks > (size_t)INT32_MAX || caps.terms > (size_t)INT32_MAX) return kNoMem;
  HG_GT_ALLOC(c, ws_ensure(ws, n, kWsGtFold, caps));
  w.plan = ws.gt_plan.p;
  w.hdr = ws.gt_hdr.p;
  w.terms = ws.gt_terms.p;
  w.ord = ws.gt_ord.p;
  w.cap = (int)caps.chunks;
  w.multi = ws.gt_multi.p;
  w.partial = ws.gt_partial.p;
  const size_t per_wg = kGtChunkTeams;
  // no more chunk workgroups than the batch can have chunks (a small batch
  // would otherwise launch thousands of workgroups that exit at once)
  const size_t need = (caps.chunks + per_wg - 1) / per_wg;
  w.chunk_grid = (int)(need < (size_t)grid ? (need ? need : 1) : (size_t)grid);
  w.chunk = gt_chunk();
  return HG_OK;
}

// The tables of `level` and the fold workspaces of one submission (inside it,
// on stream s). Lowers `level` for what the device cannot hold: tables that do
// not fit cap the context (tables never get smaller for this registry), fold
// workspaces that do not fit send this submission to the G2 fold only.
// may_build = false (service lanes): run at the built level at most; builds
// happen between batches, with the lanes drained (hg_lane_build_level)
static int gt_acquire(hg_ctx* c, Ws& ws, hipStream_t s, size_t n, const FoldCaps& caps, int& level, GtWork& w,
                      bool may_build) {
  if (!may_build && level > c->cur.gt_level) level = c->cur.gt_level;
  if (level > 0 && c->cur.gt_level < level) {
    int rc = build_fitting_locked(c, s, level);
    if (rc) return rc;
  }
  if (level > 0) {
    int rc = ensure_gt_fold(c, ws, n, caps, w);
    if (rc == kNoMem) level = 0;
    else if (rc) return rc;
  }
  return HG_OK;
}

int submission_level(hg_ctx* c, const AggBatch& b, Ws& ws, hipStream_t s, bool may_build, int& level, GtWork& gw) {
  level = gt_submission_level(c, b.n);
  gw = GtWork{};
  if (level > 0) {
    int rc = gt_acquire(c, ws, s, b.n, b.caps ? *b.caps : fold_caps_worst(c, b.n), level, gw, may_build);
    if (rc) return rc;
  }
  // a set in torus form has one fold table, the 16-key windows
  if (level > 0 && c->cur.gt_level == 2 && c->cur.torus) level = 2;
  gw.win_bits = level == 2 ? 16 : 8;
  gw.torus = level == 2 && c->cur.torus;
  return HG_OK;
}

// The fold beside the pairing kernel (default; hg_set_fold_overlap(ctx, 0) or
// HG_GT_OVERLAP=0 for new contexts runs them one after the other, with the
// comparison inside k_verify_sig): k_verify_sig at one wave per SIMD leaves
// issue slots (and LDS for one fold workgroup per CU) for the fold's waves.
bool gt_overlap() {
  static const bool on = env_int("HG_GT_OVERLAP", 1, 0, 1) != 0;
  return on;
}

void gt_prologue(hg_ctx* c, const AggBatch& b, Ws& ws, const GtWork& gw, hipStream_t s) {
  launch_agg_prologue(b.reqs, (int)b.n, (uint32_t)c->nreg, b.sigs, c->flavor, ws.pts1.p, b.codes, (int*)gw.hdr,
                      (int)(sizeof(GtHdr) / sizeof(int)), s);
}
void gt_fold(hg_ctx* c, const AggBatch& b, Ws& ws, const GtWork& gw, int32_t* codes, bool zero_hdr, hipStream_t s) {
  launch_gt_fold(b.reqs, (int)b.n, b.words, codes, (int)c->nreg, c->block_levels,
                 gw.win_bits == 16 ? c->cur.gt_win.p : c->cur.gt_w8.p, c->cur.gt_blk.p, c->gt_bi, gw, ws.gt_y.p, zero_hdr,
                 s);
}
// the pairing in its stored form (the batch's): fe[r] = FE(Miller(G2Base at -sig_r))
int pair_stored(hg_ctx* c, const AggBatch& b, Ws& ws, SigForm form, hipStream_t s) {
  PhaseTimer t(c, HG_PHASE_VERIFY, s);
  const bool ran = launch_sig_form(form, b.sigs, c->flavor, (int)b.n, c->d_lines.p, ws.sig_lines.p, ws.gt_fe.p, s);
  t.stop();
  if (!ran) {
    c->err = "aggregate batch too large for its pairing form";
    return HG_ERR_ARG;
  }
  return HG_OK;
}
// the stored FE values against gt_y: the fold's X on a torus set (the verdict bitset with it), else Y
void compare_stored(const AggBatch& b, Ws& ws, const GtWork& gw, hipStream_t s) {
  if (gw.torus) launch_tor_compare(ws.gt_fe.p, ws.gt_y.p, (int)b.n, b.codes, b.bits, s);
  else if (b.bits) launch_gt_compare_bits(ws.gt_fe.p, ws.gt_y.p, (int)b.n, b.codes, b.bits, s);
  else launch_gt_compare(ws.gt_fe.p, ws.gt_y.p, (int)b.n, b.codes, s);
}
// both: how a flow that folds first ends on a torus set (k_verify_sig's own comparison cannot be used)
static int pair_and_compare(hg_ctx* c, const AggBatch& b, Ws& ws, SigForm form, const GtWork& gw, hipStream_t s) {
  const int rc = pair_stored(c, b, ws, form, s);
  if (rc == HG_OK) compare_stored(b, ws, gw, s);
  return rc;
}

// GT path, verdicts only, the fold beside the pairing:
// s:    pairing (decodes its signatures) ............ -> wait -> compare
// side: wait -> prologue (codes, counters), plan, chunks, combine -> join
static int flow_gt_beside(hg_ctx* c, const AggBatch& b, Ws& ws, SigForm form, const GtWork& gw, hipStream_t s) {
  HG_CHECK(c, hipEventRecord(ws.ev_fork, s));
  int rc = pair_stored(c, b, ws, form, s);
  if (rc) return rc;
  HG_CHECK(c, hipStreamWaitEvent(ws.side, ws.ev_fork, 0));
  gt_prologue(c, b, ws, gw, ws.side);
  PhaseTimer fold(c, HG_PHASE_AGGREGATE, ws.side);
  gt_fold(c, b, ws, gw, b.codes, false, ws.side);
  fold.stop();
  HG_CHECK(c, hipEventRecord(ws.ev_join, ws.side));
  HG_CHECK(c, hipStreamWaitEvent(s, ws.ev_join, 0));
  compare_stored(b, ws, gw, s);
  return HG_OK;
}

// GT path, verdicts only, in sequence: level check, signature decode and the
// fold's counters in one launch, then the fold and k_verify_sig on the codes
static int flow_gt_sequence(hg_ctx* c, const AggBatch& b, Ws& ws, SigForm form, const GtWork& gw, hipStream_t s) {
  const int n = (int)b.n;
  gt_prologue(c, b, ws, gw, s);
  PhaseTimer fold(c, HG_PHASE_AGGREGATE, s);
  gt_fold(c, b, ws, gw, b.codes, false, s);
  fold.stop();
  if (gw.torus) return pair_and_compare(c, b, ws, form, gw, s);
  PhaseTimer t(c, HG_PHASE_VERIFY, s);
  launch_verify_sig(ws.pts1.p, n, c->d_lines.p, ws.gt_y.p, b.codes, s);
  t.stop();
  if (b.bits) launch_pack_verdicts(b.codes, n, b.bits, s);
  return HG_OK;
}

// The G2 fold (g2_fold: no tables, or the caller wants the aggregate keys'
// marshals), the GT fold beside it when use_gt, and (verify) the check:
// k_verify_sig against the GT fold's values, or config 2 on the G2 fold's
int flow_g2_or_mixed(hg_ctx* c, const AggBatch& b, Ws& ws, bool verify, bool use_gt, bool g2_fold, SigForm form,
                     const GtWork& gw, hipStream_t s) {
  const int n = (int)b.n;
  int32_t* d_lvl = b.lvl;
  if (!d_lvl) {
    d_lvl = ws.codes_c.p;
    launch_aggmsgs_levels(b.reqs, n, (uint32_t)c->nreg, d_lvl, s);
  }
  PhaseTimer fold(c, HG_PHASE_AGGREGATE, s);
  if (g2_fold)
    launch_aggregate(c->wsum.p, (int)c->nreg, c->blocks.p, c->block_base.data(), c->block_levels, b.reqs, n, b.words,
                     ws.order.p, ws.agg_ws.p, ws.checks.p, d_lvl, s);
  if (use_gt) gt_fold(c, b, ws, gw, d_lvl, true, s);
  fold.stop();
  if (b.agg) {
    launch_extract_pk(ws.checks.p, n, ws.pts2.p, s);
    launch_encode_g2(ws.pts2.p, n, b.agg, s);
  }
  if (verify) {
    launch_decode_g1(b.sigs, n, c->flavor, ws.pts1.p, ws.codes_b.p, s);
    launch_agg_codes(ws.codes_b.p, d_lvl, c->cur.hash_eof ? 1 : 0, n, b.codes, s);
    if (use_gt && gw.torus) {
      return pair_and_compare(c, b, ws, form, gw, s);  // the verdict bitset with it
    } else if (use_gt) {
      PhaseTimer t(c, HG_PHASE_VERIFY, s);
      launch_verify_sig(ws.pts1.p, n, c->d_lines.p, ws.gt_y.p, b.codes, s);
      t.stop();
    } else if (!c->cur.hash_eof) {
      launch_sig_into_checks(ws.pts1.p, n, ws.checks.p, s);
      PhaseTimer t(c, HG_PHASE_VERIFY, s);
      launch_verify(ws.checks.p, n, c->d_lines.p, c->cur.d_h.p, b.codes, s);
      t.stop();
    }
  }
  if (b.bits) launch_pack_verdicts(b.codes, n, b.bits, s);
  return HG_OK;
}

// The Combine fold and (verify) the pairing check of a batch on stream s,
// with the workspaces ws and the pairing policy pol: the context's own, or a
// service lane's (is_lane: outside the context's submission chain, and never
// building tables).
int aggregate_device_locked(hg_ctx* c, const AggBatch& b, bool verify, hipStream_t s, Ws& ws, const SigPolicy& pol,
                            bool is_lane) {
  if (verify && !c->cur.has_msg) {
    c->err = "hg_set_message was not called";
    return HG_ERR_ARG;
  }
  const size_t n = b.n;
  Submission sub(c, s);
  if (!is_lane) HG_CHECK(c, sub.start());
  // GT path: the verdict needs no aggregate key in G2; the G2 fold still runs
  // when the caller wants the aggregate keys' marshals
  int level = 0;
  GtWork gw{};
  if (verify) {
    int rc = submission_level(c, b, ws, s, !is_lane, level, gw);
    if (rc) return rc;
  }
  const bool use_gt = level > 0;
  const bool g2_fold = !use_gt || b.agg;
  const bool beside = use_gt && !g2_fold && pol.overlap;
  // the pairing's form: chosen once, it sizes the workspace and is what runs
  const SigForm form = sig_form(sig_env(), pol, n);
  const unsigned parts = (g2_fold ? kWsG2Fold : 0) | (b.agg ? kWsAggOut : 0) | (b.lvl ? 0 : kWsLevel) |
                         (verify ? kWsVerify : 0) | (beside ? kWsPairing | kWsSide : 0) | (gw.torus ? kWsPairing : 0);
  HG_CHECK(c, ws_ensure(ws, n, parts, {}, sig_form_ws_bytes(form, (int)n)));
  PhaseTimer all(c, HG_PHASE_SUBMIT, s);
  int rc;
  if (beside) rc = flow_gt_beside(c, b, ws, form, gw, s);
  else if (use_gt && !g2_fold) rc = flow_gt_sequence(c, b, ws, form, gw, s);
  else rc = flow_g2_or_mixed(c, b, ws, verify, use_gt, g2_fold, form, gw, s);
  if (rc) return rc;
  all.stop();
  rc = check_launch(c);
  if (rc) return rc;
  if (!is_lane) HG_CHECK(c, sub.finish());
  return HG_OK;
}

// ---------------------------------------------------------------- host pointers in
int check_host_requests(hg_ctx* c, const HostBatch& h, int32_t* lvl, FoldCaps* caps) {
  const auto add = [caps](const hg_request& r) {
    if (caps) caps->add(r.bitlen);
  };
  const size_t i = first_request_outside(h.reqs, h.n, c->nreg, h.nwords, WordsRule::kSkipLevelErrors, lvl, add);
  if (i == kNoRequest) return HG_OK;
  char buf[160];
  snprintf(buf, sizeof buf, "%s: request %zu (word offset %u, %u bits) leaves the %zu bitset words", h.who, i,
           h.reqs[i].word_offset, h.reqs[i].bitlen, h.nwords);
  c->err = buf;
  return HG_ERR_ARG;
}

int HostStage::open(const HostBatch& h, bool want_keys) {
  HG_CHECK(c, hipSetDevice(c->device));
  HG_CHECK(c, c->reqs.ensure(h.n));
  HG_CHECK(c, c->words.ensure(h.nwords ? h.nwords : 1));
  HG_CHECK(c, c->codes_a.ensure(h.n));
  if (h.sigs) HG_CHECK(c, c->bytes_b.ensure(h.n * 64));
  if (want_keys) {
    HG_CHECK(c, c->bytes_a.ensure(h.n * 128));
    d_keys = c->bytes_a.p;
  }
  HG_CHECK(c, sub.start());
  HG_CHECK(c, hipMemcpyAsync(c->reqs.p, h.reqs, h.n * sizeof(hg_request), hipMemcpyHostToDevice, c->stream));
  if (h.nwords) HG_CHECK(c, hipMemcpyAsync(c->words.p, h.words, h.nwords * 8, hipMemcpyHostToDevice, c->stream));
  if (h.sigs) HG_CHECK(c, hipMemcpyAsync(c->bytes_b.p, h.sigs, h.n * 64, hipMemcpyHostToDevice, c->stream));
  return HG_OK;
}

int HostStage::close(const HostBatch& h, const int32_t* d_codes, int32_t* codes, uint8_t* keys_out) {
  if (keys_out) HG_CHECK(c, hipMemcpyAsync(keys_out, d_keys, h.n * 128, hipMemcpyDeviceToHost, c->stream));
  HG_CHECK(c, hipMemcpyAsync(codes, d_codes, h.n * 4, hipMemcpyDeviceToHost, c->stream));
  HG_CHECK(c, sub.finish());
  HG_CHECK(c, hipStreamSynchronize(c->stream));
  return HG_OK;
}

// The request of VerifyMultiSignature (crypto.go:121-137): the range [0, N),
// whose level check is the reference's size check (crypto.go:121-124), renamed
// HG_ERR_MULTI_SIZES by the caller. The two callers rename differently, and
// both stand as they are: hg_verify_multisig gives every request with
// bitlen != N that code, whatever its signature's code was;
// hg_verify_multisig_msgs renames HG_ERR_LEVEL only, so there a signature that
// does not unmarshal keeps its own code. Which of the two is crypto.go's order
// is open.
std::vector<hg_request> multisig_requests(const hg_ctx* c, const uint32_t* bitlens, const uint32_t* word_offsets,
                                          size_t n) {
  std::vector<hg_request> reqs(n);
  for (size_t i = 0; i < n; i++) reqs[i] = hg_request{0u, bitlens[i], (uint32_t)c->nreg, word_offsets[i]};
  return reqs;
}

// verify: hg_verify_aggregate*'s batch; else hg_aggregate_pk's (no signatures, the codes are the fold's level codes)
static int aggregate_host_locked(hg_ctx* c, const HostBatch& h, int32_t* codes, uint8_t* agg_out, bool verify) {
  std::vector<int32_t> lvl(h.n);
  FoldCaps caps;  // exact bounds: the host knows every request's size
  int rc = check_host_requests(c, h, lvl.data(), &caps);
  if (rc) return rc;
  HostStage st(c);
  rc = st.open(h, agg_out != nullptr);
  if (rc == HG_OK) rc = st.put(c->ws.codes_c, lvl.data(), h.n);
  if (rc) return rc;
  AggBatch b = st.batch(h);
  b.lvl = c->ws.codes_c.p;
  b.caps = &caps;
  rc = aggregate_device_locked(c, b, verify, c->stream, c->ws, c->pol, false);
  if (rc == HG_OK) rc = st.close(h, verify ? b.codes : b.lvl, codes, agg_out);
  if (rc) return rc;
  if (agg_out) {
    // the reference has no aggregate for level errors / empty bitsets: zero them
    for (size_t i = 0; i < h.n; i++)
      if (lvl[i] != HG_OK || codes[i] == HG_ERR_EMPTY_AGG) memset(agg_out + 128 * i, 0, 128);
  }
  return HG_OK;
}

extern "C" {

int hg_set_fold_overlap(hg_ctx* c, int on) {
  if (!c) return HG_ERR_ARG;
  std::lock_guard<std::mutex> g(c->mu);
  c->pol.overlap = on != 0;
  return HG_OK;
}

int hg_set_verify_split(hg_ctx* c, int on) {
  if (!c) return HG_ERR_ARG;
  std::lock_guard<std::mutex> g(c->mu);
  c->verify_split = on != 0;
  return HG_OK;
}

int hg_verify_aggregate_device(hg_ctx* c, const hg_request* d_reqs, size_t n, const uint64_t* d_words,
                               const uint8_t* d_sigs, int32_t* d_codes, uint8_t* d_agg_pk_out, void* stream) {
  if (!c || (n && (!d_reqs || !d_sigs || !d_codes)) || n > (size_t)INT32_MAX) return HG_ERR_ARG;
  if (n == 0) return HG_OK;
  std::lock_guard<std::mutex> g(c->mu);
  HG_CHECK(c, hipSetDevice(c->device));
  hipStream_t s = stream ? (hipStream_t)stream : c->stream;
  return aggregate_device_locked(c, AggBatch{d_reqs, n, d_words, d_sigs, d_codes, d_agg_pk_out}, true, s, c->ws, c->pol,
                                 false);
}

int hg_verify_aggregate_device_bits(hg_ctx* c, const hg_request* d_reqs, size_t n, const uint64_t* d_words,
                                    const uint8_t* d_sigs, int32_t* d_codes, uint8_t* d_bits, void* stream) {
  if (!c || (n && (!d_reqs || !d_sigs || !d_codes || !d_bits)) || n > (size_t)INT32_MAX) return HG_ERR_ARG;
  if (n == 0) return HG_OK;
  std::lock_guard<std::mutex> g(c->mu);
  HG_CHECK(c, hipSetDevice(c->device));
  hipStream_t s = stream ? (hipStream_t)stream : c->stream;
  return aggregate_device_locked(c, AggBatch{d_reqs, n, d_words, d_sigs, d_codes, nullptr, nullptr, d_bits}, true, s,
                                 c->ws, c->pol, false);
}

int hg_verify_aggregate(hg_ctx* c, const hg_request* reqs, size_t n, const uint64_t* words, size_t nwords,
                        const uint8_t* sigs, int32_t* codes, uint8_t* agg_pk_out) {
  if (!c || (n && (!reqs || !sigs || !codes)) || n > (size_t)INT32_MAX) return HG_ERR_ARG;
  if (n == 0) return HG_OK;
  std::lock_guard<std::mutex> g(c->mu);
  return aggregate_host_locked(c, HostBatch{"hg_verify_aggregate", reqs, n, words, nwords, sigs}, codes, agg_pk_out,
                               true);
}

int hg_verify_aggregate_msg(hg_ctx* c, const uint8_t* msg, size_t len, const hg_request* reqs, size_t n,
                            const uint64_t* words, size_t nwords, const uint8_t* sigs, int32_t* codes,
                            uint8_t* agg_pk_out) {
  if (!c || (!msg && len) || (n && (!reqs || !sigs || !codes)) || n > (size_t)INT32_MAX) return HG_ERR_ARG;
  std::lock_guard<std::mutex> g(c->mu);
  int rc = set_message_locked(c, msg, len);
  if (rc != HG_OK && rc != HG_ERR_HASH_EOF) return rc;
  if (n == 0) return HG_OK;
  return aggregate_host_locked(c, HostBatch{"hg_verify_aggregate_msg", reqs, n, words, nwords, sigs}, codes, agg_pk_out,
                               true);
}

int hg_verify_multisig(hg_ctx* c, const uint32_t* bitlens, const uint32_t* word_offsets, size_t n,
                       const uint64_t* words, size_t nwords, const uint8_t* sigs, int32_t* codes) {
  if (!c || (n && (!bitlens || !word_offsets || !sigs || !codes)) || n > (size_t)INT32_MAX) return HG_ERR_ARG;
  if (n == 0) return HG_OK;
  std::lock_guard<std::mutex> g(c->mu);
  // crypto.go:121-124: the bitset must span the registry; the rest is
  // verifySignature over the range [0, N) (crypto.go:125-136)
  const std::vector<hg_request> reqs = multisig_requests(c, bitlens, word_offsets, n);
  int rc = aggregate_host_locked(c, HostBatch{"hg_verify_multisig", reqs.data(), n, words, nwords, sigs}, codes, nullptr,
                                 true);
  if (rc) return rc;
  for (size_t i = 0; i < n; i++)
    if (bitlens[i] != c->nreg) codes[i] = HG_ERR_MULTI_SIZES;
  return HG_OK;
}

// The fold alone, for the value-level tests: submission_level's window width
// and form over the tables as built, `chunk` terms per chunk, every workspace
// local and sized for that chunk (FoldCaps and ensure_gt_fold follow gt_chunk()).
int hg_debug_gt_fold(hg_ctx* c, const hg_request* reqs, size_t n, const uint64_t* words, size_t nwords, int chunk,
                     uint32_t* y, int32_t* codes) {
  if (!c || !reqs || !y || !codes || (!words && nwords) || n == 0 || n > ((size_t)1 << 20) || chunk < 1 || chunk > 64)
    return HG_ERR_ARG;
  std::lock_guard<std::mutex> g(c->mu);
  if (c->cur.gt_level < 1 || c->nreg == 0) {
    c->err = "hg_debug_gt_fold: no tables are built";
    return HG_ERR_ARG;
  }
  std::vector<int32_t> lvl(n);
  int rc = check_host_requests(c, HostBatch{"hg_debug_gt_fold", reqs, n, words, nwords, nullptr}, lvl.data(), nullptr);
  if (rc) return rc;
  // capacities: at most 8 nonzero windows per registry-aligned word of the
  // range (either width, the shift included) and the block term
  size_t terms = 0, chunks = 0;
  for (size_t i = 0; i < n; i++) {
    if (lvl[i] != HG_OK) continue;
    const size_t m = 8 * (((size_t)reqs[i].bitlen + 15 + 63) / 64) + 1;
    terms += m;
    chunks += (m + chunk - 1) / chunk;
  }
  if (terms > (size_t)INT32_MAX) return HG_ERR_ARG;
  HG_CHECK(c, hipSetDevice(c->device));
  DevBuf<hg_request> d_reqs;
  DevBuf<uint64_t> d_words;
  DevBuf<int32_t> d_codes;
  DevBuf<GtReq> plan;
  DevBuf<GtHdr> hdr;
  DevBuf<uint32_t> d_terms;
  DevBuf<int2> ord;
  DevBuf<int> multi;
  DevBuf<Gt> partial, d_y;
  HG_CHECK(c, d_reqs.ensure(n));
  HG_CHECK(c, d_words.ensure(nwords ? nwords : 1));
  HG_CHECK(c, d_codes.ensure(n));
  HG_CHECK(c, plan.ensure(n));
  HG_CHECK(c, hdr.ensure(1));
  HG_CHECK(c, d_terms.ensure(terms ? terms : 1));
  HG_CHECK(c, ord.ensure(chunks ? chunks : 1));
  HG_CHECK(c, multi.ensure(2 * n));
  HG_CHECK(c, partial.ensure(chunks ? chunks : 1));
  HG_CHECK(c, d_y.ensure(n));
  GtWork w{};
  w.plan = plan.p;
  w.hdr = hdr.p;
  w.terms = d_terms.p;
  w.ord = ord.p;
  w.cap = (int)(chunks ? chunks : 1);
  w.multi = multi.p;
  w.partial = partial.p;
  const size_t need = (chunks + kGtChunkTeams - 1) / kGtChunkTeams;
  w.chunk_grid = (int)(need < 4096 ? (need ? need : 1) : 4096);
  w.chunk = chunk;
  // submission_level's rule over the built tables: the pinned level if lower, but a torus set has one fold table
  int level = c->cur.gt_level;
  if (c->pinned_level >= 1 && c->pinned_level < level) level = c->pinned_level;
  if (c->cur.gt_level == 2 && c->cur.torus) level = 2;
  w.win_bits = level == 2 ? 16 : 8;
  w.torus = level == 2 && c->cur.torus;
  hipStream_t s = c->stream;
  Submission sub(c, s);
  HG_CHECK(c, sub.start());
  HG_CHECK(c, hipMemcpyAsync(d_reqs.p, reqs, n * sizeof(hg_request), hipMemcpyHostToDevice, s));
  if (nwords) HG_CHECK(c, hipMemcpyAsync(d_words.p, words, nwords * 8, hipMemcpyHostToDevice, s));
  HG_CHECK(c, hipMemsetAsync(d_y.p, 0, n * sizeof(Gt), s));
  launch_aggmsgs_levels(d_reqs.p, (int)n, (uint32_t)c->nreg, d_codes.p, s);
  launch_gt_fold(d_reqs.p, (int)n, d_words.p, d_codes.p, (int)c->nreg, c->block_levels,
                 w.win_bits == 16 ? c->cur.gt_win.p : c->cur.gt_w8.p, c->cur.gt_blk.p, c->gt_bi, w, d_y.p, true, s);
  rc = check_launch(c);
  HG_CHECK(c, sub.finish());
  // the local workspaces are freed on return: nothing may still be running
  HG_CHECK(c, hipStreamSynchronize(s));
  if (rc) return rc;
  HG_CHECK(c, hipMemcpy(y, d_y.p, n * sizeof(Gt), hipMemcpyDeviceToHost));
  HG_CHECK(c, hipMemcpy(codes, d_codes.p, n * 4, hipMemcpyDeviceToHost));
  return HG_OK;
}

int hg_aggregate_pk(hg_ctx* c, const hg_request* reqs, size_t n, const uint64_t* words, size_t nwords,
                    uint8_t* agg_pk_out, int32_t* codes) {
  if (!c || (n && (!reqs || !agg_pk_out || !codes)) || n > (size_t)INT32_MAX) return HG_ERR_ARG;
  if (n == 0) return HG_OK;
  std::lock_guard<std::mutex> g(c->mu);
  return aggregate_host_locked(c, HostBatch{"hg_aggregate_pk", reqs, n, words, nwords, nullptr}, codes, agg_pk_out,
                               false);
}

}  // extern "C"
