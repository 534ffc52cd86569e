// hg_aggregate.cpp — aggregate verification (processing.go verifySignature)
// behind include/handel_gpu.h: the GT table policy of a context, the Combine
// fold and pairing check of a batch (aggregate_device_locked), the calls that
// steer them, and the service lanes, which submit batches through the same
// body on their own workspaces. State and helpers shared with hg_api.cpp and
// hg_intake.cpp are in hg_ctx.h.
#include <cstring>

#include "hg_aggregate.h"

namespace {

// final = sig decode error > level error > hash EOF > empty aggregate > (verify)
__global__ void k_agg_codes(const int32_t* sig_codes, const int32_t* lvl_codes, int hash_eof, int n, int32_t* out) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  int32_t c = sig_codes[i];
  if (c == HG_OK && lvl_codes[i] == HG_ERR_LEVEL) c = HG_ERR_LEVEL;
  if (c == HG_OK && hash_eof) c = HG_ERR_HASH_EOF;
  if (c == HG_OK) c = lvl_codes[i];
  out[i] = c;
}
}  // namespace

// host-side request validation: the level check of processing.go:350-352
void level_codes(hg_ctx* c, const hg_request* reqs, size_t n, std::vector<int32_t>& out) {
  out.resize(n);
  for (size_t i = 0; i < n; i++) {
    const hg_request& r = reqs[i];
    bool ok = r.bitlen == r.level_size && (size_t)r.offset + r.bitlen <= c->nreg;
    out[i] = ok ? HG_OK : HG_ERR_LEVEL;
  }
}

// The GT tables. Level 1 (e(H, pk_i) for every key, 8-key window subset
// products, aligned block products: ≈ 3 ms and 61 MB for 4000 keys) saves
// ≈ 0.6 ms per 4096-request batch against the G2 fold (config 3), so it pays
// for itself after ≈ 20 k requests of one message; level 2 (16-key windows:
// ≈ 12.5 ms more and ≈ 1.97 MB of HBM per key, registries up to 16384 keys)
// saves another ≈ 0.05 ms per batch and pays off after ≈ 1 M requests. The
// thresholds are those break-even volumes (a rent-or-buy rule: at most about
// twice the cost of the better choice in hindsight). A message or registry
// change drops the tables and restarts the count. hg_prepare_aggregate builds
// the top level at once (serving). hg_set_aggregate_level pins a level per
// context (0 = G2 fold only); HG_GT_LEVEL=0/1/2 (HG_AGG_PATH=g2 = 0) is the
// pinned level of new contexts (tests and A/B runs).
//
// The tables are a cache, never a requirement: a level whose tables (or fold
// workspaces) the device cannot hold, or that exceeds the context's table
// budget, lowers the context's cap and the submission runs at the level below
// (down to the G2 fold, which needs no tables). A registry with a key outside
// G2 stays at level 0 (the GT product equals e(H, sum) only on G2).
static constexpr size_t kGtMaxRegistry = 16384;
static constexpr size_t kGtLevel1Requests = 16384;
static constexpr size_t kGtLevel2Requests = (size_t)1 << 20;
static constexpr int kNoMem = -1;       // internal: an allocation of the GT path failed
static constexpr int kOverBudget = -2;  // internal: a table level exceeds hg_set_table_budget
int gt_forced_level() {
  static const int lvl = [] {
    const char* p = getenv("HG_AGG_PATH");
    if (p && strcmp(p, "g2") == 0) return 0;
    const char* e = getenv("HG_GT_LEVEL");
    if (!e) return -1;
    const int v = atoi(e);
    return v >= 0 && v <= 2 ? v : -1;
  }();
  return lvl;
}
// the registry's G2 membership count, waiting for its check if still running
static int resolve_subgroup(hg_ctx* c) {
  if (!c->sub_pending) return HG_OK;
  int cnt = 0;
  HG_CHECK(c, hipEventSynchronize(c->ev_sub));
  HG_CHECK(c, hipMemcpy(&cnt, c->sub_count.p, sizeof cnt, hipMemcpyDeviceToHost));
  c->reg_non_g2 = (size_t)cnt;
  c->sub_pending = false;
  return HG_OK;
}
// the highest table level the registry may use (the membership check must be resolved)
static int gt_max_level(const hg_ctx* c) {
  if (c->reg_non_g2 || c->sub_pending) return 0;
  const int top = c->nreg <= kGtMaxRegistry ? 2 : 1;
  return top < c->gt_cap ? top : c->gt_cap;
}

// an allocation of the GT path: out of device memory -> kNoMem (the caller
// falls back to a lower level), any other failure -> HG_ERR_DEVICE
#define HG_GT_ALLOC(ctx, expr)                                                     \
  do {                                                                             \
    hipError_t e_ = (expr);                                                        \
    if (e_ == hipErrorOutOfMemory) {                                               \
      (void)hipGetLastError(); /* not sticky: keep it out of check_launch */       \
      return kNoMem;                                                               \
    }                                                                              \
    if (e_ != hipSuccess) {                                                        \
      (ctx)->err = std::string(#expr) + ": " + hipGetErrorString(e_);              \
      return HG_ERR_DEVICE;                                                        \
    }                                                                              \
  } while (0)

// bytes of the tables of `level` (cumulative) for an n-key registry
static size_t gt_block_count(const hg_ctx* c, int* cnt) {
  size_t total = 0;
  for (int k = 4; k <= c->block_levels && k < 24; k++) {
    const size_t v = (c->nreg + ((size_t)1 << k) - 1) >> k;
    if (cnt) cnt[k] = (int)v;
    total += v;
  }
  return total;
}
static size_t gt_table_bytes(const hg_ctx* c, int level) {
  const size_t n = c->nreg, nwin8 = (n + 7) / 8, nwin16 = (n + 15) / 16;
  size_t b = 0;
  if (level >= 1) b += (n + nwin8 * 256 + gt_block_count(c, nullptr)) * sizeof(Gt);
  if (level >= 2) b += nwin16 * 65536 * sizeof(Gt);
  return b;
}

// The level-2 fold tables (the 16-key windows and the blocks) to torus form,
// in place, unless HG_GT_TORUS=0 or an entry has none: a registry may hold
// keys whose sum over some window subset or block is zero (k and r - k), and
// e(H, 0) = 1 has no torus form. The scan runs first and the host reads its
// flag, so a set is converted whole or not at all. (The flag word is the
// registry's membership counter, idle once resolve_subgroup has read it.)
static bool gt_torus_enabled() {
  static const bool on = env_int("HG_GT_TORUS", 1, 0, 1) != 0;
  return on;
}
static int convert_torus_locked(hg_ctx* c, hipStream_t s, size_t nwin) {
  c->cur.torus = false;
  if (!gt_torus_enabled()) return HG_OK;
  const size_t nblk = gt_block_count(c, nullptr);
  HG_CHECK(c, c->sub_count.ensure(1));
  int degenerate = 0;
  launch_tor_scan(c->cur.gt_win.p, nwin, c->cur.gt_blk.p, nblk, (int)c->nreg, c->sub_count.p, s);
  HG_CHECK(c, hipMemcpyAsync(&degenerate, c->sub_count.p, sizeof degenerate, hipMemcpyDeviceToHost, s));
  HG_CHECK(c, hipStreamSynchronize(s));
  if (degenerate) return HG_OK;
  launch_tor_convert(c->cur.gt_win.p, nwin, c->cur.gt_blk.p, nblk, (int)c->nreg, s);
  int rc = check_launch(c);
  if (rc) return rc;
  c->cur.torus = true;
  return HG_OK;
}

// builds the tables up to `level` on stream s (inside a submission); kNoMem /
// kOverBudget before any launch of the level that could not be held. The
// budget covers both messages' tables.
static int build_gt_locked(hg_ctx* c, hipStream_t s, int level) {
  const int n = (int)c->nreg;
  const int nwin8 = (n + 7) / 8, nwin16 = (n + 15) / 16;
  if (c->cur.gt_level < 1 && level >= 1) {
    if (gt_table_bytes(c, 1) + c->alt.table_bytes() > c->table_budget) return kOverBudget;
    int cnt[24] = {0};
    const size_t total = gt_block_count(c, cnt);
    int base = 0;
    for (int k = 4; k <= c->block_levels && k < 24; k++) {
      c->gt_bi.base[k] = base;
      base += cnt[k];
    }
    HG_GT_ALLOC(c, c->cur.gt_key.ensure(n));
    HG_GT_ALLOC(c, c->cur.gt_w8.ensure((size_t)nwin8 * 256));
    if (total) HG_GT_ALLOC(c, c->cur.gt_blk.ensure(total));
    launch_gt_keys(c->reg.p, n, c->d_lines.p, c->cur.d_h.p, c->cur.gt_key.p, s);
    launch_gt_windows8(c->cur.gt_key.p, n, c->cur.gt_w8.p, nwin8, s);
    for (int k = 4; k <= c->block_levels && k < 24; k++) {
      if (k == 4) launch_gt_blocks(c->cur.gt_w8.p + 255, 256, nwin8, c->cur.gt_blk.p + c->gt_bi.base[4], cnt[4], s);
      else launch_gt_blocks(c->cur.gt_blk.p + c->gt_bi.base[k - 1], 1, cnt[k - 1], c->cur.gt_blk.p + c->gt_bi.base[k], cnt[k], s);
    }
    int rc = check_launch(c);
    if (rc) return rc;
    c->cur.gt_level = 1;
  }
  if (c->cur.gt_level < 2 && level >= 2) {
    if (gt_table_bytes(c, 2) + c->alt.table_bytes() > c->table_budget) return kOverBudget;
    HG_GT_ALLOC(c, c->cur.gt_win.ensure((size_t)nwin16 * 65536));
    launch_gt_windows16(c->cur.gt_w8.p, nwin8, c->cur.gt_win.p, nwin16, s);
    int rc = check_launch(c);
    if (rc) return rc;
    rc = convert_torus_locked(c, s, (size_t)nwin16 * 65536);
    if (rc) return rc;
    c->cur.gt_level = 2;
  }
  return HG_OK;
}

// caps the context's table level at `cap` and frees the tables above it; an
// out-of-memory cap also holds across later budget changes (oom_cap)
static void gt_lower_cap(hg_ctx* c, int cap, bool oom) {
  if (cap < 0) cap = 0;
  if (cap < c->gt_cap) c->gt_cap = cap;
  if (oom && cap < c->oom_cap) c->oom_cap = cap;
  // a torus set's block table is of no use without its 16-key windows: the
  // lower level is rebuilt from the keys
  if (c->gt_cap < 2 && c->cur.gt_level == 2 && c->cur.torus) c->cur.drop_tables();
  if (c->gt_cap < 2) c->cur.gt_win.reset();
  if (c->gt_cap < 1) c->cur.drop_tables();
  if (c->cur.gt_level > c->gt_cap) c->cur.gt_level = c->gt_cap;
}

// builds up to `level` (lowering it to what fits: the cached message's tables
// go first, then the cap); HG_OK with `level` = what was built
static int build_fitting_locked(hg_ctx* c, hipStream_t s, int& level) {
  while (level > c->cur.gt_level) {
    int rc = build_gt_locked(c, s, level);
    if (rc == kNoMem || rc == kOverBudget) {
      if (c->alt.drop_tables()) continue;
      gt_lower_cap(c, c->cur.gt_level < level ? c->cur.gt_level : level - 1, rc == kNoMem);
      level = level < c->gt_cap ? level : c->gt_cap;
      continue;
    }
    if (rc) return rc;
  }
  return HG_OK;
}

// the table level an aggregate submission of n requests runs at (counting
// them towards the volume policy)
int gt_submission_level(hg_ctx* c, size_t n) {
  if (c->cur.hash_eof || c->nreg == 0) return 0;
  // a GT level needs the registry's G2 membership (resolved only then)
  const bool wants_gt = c->pinned_level > 0 || c->cur.gt_level > 0 || c->cur.gt_requests + n >= kGtLevel1Requests;
  if (wants_gt && resolve_subgroup(c) != HG_OK) return 0;
  const int top = gt_max_level(c);
  if (c->pinned_level >= 0) return c->pinned_level < top ? c->pinned_level : top;
  c->cur.gt_requests += n;
  int want = c->cur.gt_requests >= kGtLevel2Requests ? 2 : (c->cur.gt_requests >= kGtLevel1Requests ? 1 : 0);
  if (want < c->cur.gt_level) want = c->cur.gt_level;
  return want < top ? want : top;
}

// GT fold workspaces. A request of b bits has at most 8 nonzero 8-bit (4
// 16-bit) windows per registry-aligned 64-bit word of its range, plus the
// block term of a complemented fold.
// Fold schedule: terms per chunk and k_gt_chunks workgroups (HG_GT_CHUNK /
// HG_GT_GRID override them for tuning runs).
static int gt_chunk() {
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
// a lane's largest batch: n requests over max_words bitset words
static FoldCaps fold_caps_lane(size_t n, size_t max_words) {
  const size_t terms = 8 * (max_words + n) + n;  // sum of fold_terms_bound over the batch
  return FoldCaps{terms, terms / (size_t)gt_chunk() + n};
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
int gt_acquire(hg_ctx* c, Ws& ws, hipStream_t s, size_t n, const FoldCaps& caps, int& level, GtWork& w,
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

// The fold beside the pairing kernel (default; hg_set_fold_overlap(ctx, 0) or
// HG_GT_OVERLAP=0 for new contexts runs them one after the other, with the
// comparison inside k_verify_sig): k_verify_sig at one wave per SIMD leaves
// issue slots (and LDS for one fold workgroup per CU) for the fold's waves.
bool gt_overlap() {
  static const bool on = env_int("HG_GT_OVERLAP", 1, 0, 1) != 0;
  return on;
}

// the level check of processing.go:350-352 on the device
__global__ void k_level_codes(const hg_request* r, int n, uint32_t nreg, int32_t* out) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  bool ok = r[i].bitlen == r[i].level_size && (uint64_t)r[i].offset + r[i].bitlen <= nreg;
  out[i] = ok ? HG_OK : HG_ERR_LEVEL;
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
    k_level_codes<<<nb(b.n), 256, 0, s>>>(b.reqs, n, (uint32_t)c->nreg, d_lvl);
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
    k_agg_codes<<<nb(b.n), 256, 0, s>>>(ws.codes_b.p, d_lvl, c->cur.hash_eof ? 1 : 0, n, b.codes);
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
static int aggregate_device_locked(hg_ctx* c, const AggBatch& b, bool verify, hipStream_t s, Ws& ws,
                                   const SigPolicy& pol, bool is_lane) {
  if (verify && !c->cur.has_msg) {
    c->err = "hg_set_message was not called";
    return HG_ERR_ARG;
  }
  const size_t n = b.n;
  Submission sub(c, s);
  if (!is_lane) HG_CHECK(c, sub.start());
  // GT path: the verdict needs no aggregate key in G2; the G2 fold still runs
  // when the caller wants the aggregate keys' marshals
  int level = verify ? gt_submission_level(c, n) : 0;
  GtWork gw{};
  if (level > 0) {
    int rc = gt_acquire(c, ws, s, n, b.caps ? *b.caps : fold_caps_worst(c, n), level, gw, !is_lane);
    if (rc) return rc;
  }
  // a set in torus form has one fold table, the 16-key windows
  if (level > 0 && c->cur.gt_level == 2 && c->cur.torus) level = 2;
  gw.win_bits = level == 2 ? 16 : 8;
  gw.torus = level == 2 && c->cur.torus;
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

static int aggregate_host_locked(hg_ctx* c, const hg_request* reqs, size_t n, const uint64_t* words, size_t nwords,
                                 const uint8_t* sigs, int32_t* codes, uint8_t* agg_out, bool verify) {
  HG_CHECK(c, hipSetDevice(c->device));
  std::vector<int32_t> lvl;
  level_codes(c, reqs, n, lvl);
  FoldCaps caps;  // exact bounds: the host knows every request's size
  for (size_t i = 0; i < n; i++) {
    if (lvl[i] != HG_OK) continue;
    if ((size_t)reqs[i].word_offset + (reqs[i].bitlen + 63) / 64 > nwords) {
      c->err = "request words out of range";
      return HG_ERR_ARG;
    }
    caps.add(reqs[i].bitlen);
  }
  HG_CHECK(c, c->reqs.ensure(n));
  HG_CHECK(c, c->words.ensure(nwords ? nwords : 1));
  HG_CHECK(c, c->codes_a.ensure(n));
  HG_CHECK(c, c->ws.codes_c.ensure(n));
  uint8_t* d_agg = nullptr;
  if (agg_out) {
    HG_CHECK(c, c->bytes_a.ensure(n * 128));
    d_agg = c->bytes_a.p;
  }
  if (verify) HG_CHECK(c, c->bytes_b.ensure(n * 64));
  Submission sub(c, c->stream);
  HG_CHECK(c, sub.start());
  HG_CHECK(c, hipMemcpyAsync(c->reqs.p, reqs, n * sizeof(hg_request), hipMemcpyHostToDevice, c->stream));
  if (nwords) HG_CHECK(c, hipMemcpyAsync(c->words.p, words, nwords * 8, hipMemcpyHostToDevice, c->stream));
  HG_CHECK(c, hipMemcpyAsync(c->ws.codes_c.p, lvl.data(), n * 4, hipMemcpyHostToDevice, c->stream));
  if (verify) HG_CHECK(c, hipMemcpyAsync(c->bytes_b.p, sigs, n * 64, hipMemcpyHostToDevice, c->stream));
  const AggBatch b{c->reqs.p, n, c->words.p, verify ? c->bytes_b.p : nullptr, c->codes_a.p, d_agg, c->ws.codes_c.p,
                   nullptr, &caps};
  int rc = aggregate_device_locked(c, b, verify, c->stream, c->ws, c->pol, false);
  if (rc) return rc;
  if (agg_out) HG_CHECK(c, hipMemcpyAsync(agg_out, d_agg, n * 128, hipMemcpyDeviceToHost, c->stream));
  HG_CHECK(c, hipMemcpyAsync(codes, verify ? c->codes_a.p : c->ws.codes_c.p, n * 4, hipMemcpyDeviceToHost, c->stream));
  HG_CHECK(c, sub.finish());
  HG_CHECK(c, hipStreamSynchronize(c->stream));
  if (agg_out) {
    // the reference has no aggregate for level errors / empty bitsets: zero them
    for (size_t i = 0; i < n; i++)
      if (lvl[i] != HG_OK || codes[i] == HG_ERR_EMPTY_AGG) memset(agg_out + 128 * i, 0, 128);
  }
  return HG_OK;
}

// builds the tables up to `want` (-1: the highest the registry, the pin and
// the device allow), synchronously
static int prepare_aggregate_locked(hg_ctx* c, int want = -1) {
  if (!c->cur.has_msg || c->nreg == 0) {
    c->err = "hg_prepare_aggregate: needs a message and a registry";
    return HG_ERR_ARG;
  }
  if (c->cur.hash_eof) return HG_ERR_HASH_EOF;
  int src = resolve_subgroup(c);
  if (src) return src;
  int level = gt_max_level(c);
  if (c->pinned_level >= 0 && c->pinned_level < level) level = c->pinned_level;
  if (want >= 0 && want < level) level = want;
  if (c->cur.gt_level >= level) return HG_OK;
  HG_CHECK(c, hipSetDevice(c->device));
  Submission sub(c, c->stream);
  HG_CHECK(c, sub.start());
  // the highest level the device (and the table budget) can hold
  int rc = build_fitting_locked(c, c->stream, level);
  if (rc) return rc;
  HG_CHECK(c, sub.finish());
  HG_CHECK(c, hipStreamSynchronize(c->stream));
  return HG_OK;
}

extern "C" {

int hg_prepare_aggregate(hg_ctx* c) {
  if (!c) return HG_ERR_ARG;
  std::lock_guard<std::mutex> g(c->mu);
  return prepare_aggregate_locked(c);
}

int hg_prepare_aggregate_msg(hg_ctx* c, const uint8_t* msg, size_t len) {
  if (!c || (!msg && len)) return HG_ERR_ARG;
  std::lock_guard<std::mutex> g(c->mu);
  int rc = set_message_locked(c, msg, len);
  if (rc) return rc;
  return prepare_aggregate_locked(c);
}

int hg_set_aggregate_level(hg_ctx* c, int level) {
  if (!c || level < -1 || level > 2) return HG_ERR_ARG;
  std::lock_guard<std::mutex> g(c->mu);
  c->pinned_level = level;
  return HG_OK;
}

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

int hg_set_table_budget(hg_ctx* c, size_t bytes) {
  if (!c) return HG_ERR_ARG;
  std::lock_guard<std::mutex> g(c->mu);
  c->table_budget = bytes;
  // drop the built tables the new budget no longer covers (the cached
  // message's first); the cap is re-evaluated against the budget by the next
  // build, but never above what an out-of-memory failure left (oom_cap)
  if (gt_table_bytes(c, c->cur.gt_level) + c->alt.table_bytes() > bytes) c->alt.drop_tables();
  if (c->cur.gt_level >= 1 && gt_table_bytes(c, c->cur.gt_level) > bytes)
    gt_lower_cap(c, gt_table_bytes(c, 1) <= bytes ? 1 : 0, false);
  c->gt_cap = c->oom_cap;
  return HG_OK;
}

size_t hg_registry_non_g2(hg_ctx* c) {
  if (!c) return 0;
  std::lock_guard<std::mutex> g(c->mu);
  if (resolve_subgroup(c) != HG_OK) return 0;
  return c->reg_non_g2;
}

int hg_aggregate_tables(hg_ctx* c) {
  if (!c) return 0;
  std::lock_guard<std::mutex> g(c->mu);
  return c->cur.gt_level;
}

int hg_aggregate_tables_torus(hg_ctx* c) {
  if (!c) return 0;
  std::lock_guard<std::mutex> g(c->mu);
  return c->cur.gt_level == 2 && c->cur.torus ? 1 : 0;
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
  return aggregate_host_locked(c, reqs, n, words, nwords, sigs, codes, agg_pk_out, true);
}

int hg_verify_aggregate_msg(hg_ctx* c, const uint8_t* msg, size_t len, const hg_request* reqs, size_t n,
                            const uint64_t* words, size_t nwords, const uint8_t* sigs, int32_t* codes,
                            uint8_t* agg_pk_out) {
  if (!c || (!msg && len) || (n && (!reqs || !sigs || !codes)) || n > (size_t)INT32_MAX) return HG_ERR_ARG;
  std::lock_guard<std::mutex> g(c->mu);
  int rc = set_message_locked(c, msg, len);
  if (rc != HG_OK && rc != HG_ERR_HASH_EOF) return rc;
  if (n == 0) return HG_OK;
  return aggregate_host_locked(c, reqs, n, words, nwords, sigs, codes, agg_pk_out, true);
}

int hg_verify_multisig(hg_ctx* c, const uint32_t* bitlens, const uint32_t* word_offsets, size_t n,
                       const uint64_t* words, size_t nwords, const uint8_t* sigs, int32_t* codes) {
  if (!c || (n && (!bitlens || !word_offsets || !sigs || !codes)) || n > (size_t)INT32_MAX) return HG_ERR_ARG;
  if (n == 0) return HG_OK;
  std::lock_guard<std::mutex> g(c->mu);
  // crypto.go:121-124: the bitset must span the registry; the rest is
  // verifySignature over the range [0, N) (crypto.go:125-136)
  std::vector<hg_request> reqs(n);
  for (size_t i = 0; i < n; i++) reqs[i] = hg_request{0u, bitlens[i], (uint32_t)c->nreg, word_offsets[i]};
  int rc = aggregate_host_locked(c, reqs.data(), n, words, nwords, sigs, codes, nullptr, true);
  if (rc) return rc;
  for (size_t i = 0; i < n; i++)
    if (bitlens[i] != c->nreg) codes[i] = HG_ERR_MULTI_SIZES;
  return HG_OK;
}

int hg_aggregate_pk(hg_ctx* c, const hg_request* reqs, size_t n, const uint64_t* words, size_t nwords,
                    uint8_t* agg_pk_out, int32_t* codes) {
  if (!c || (n && (!reqs || !agg_pk_out || !codes)) || n > (size_t)INT32_MAX) return HG_ERR_ARG;
  if (n == 0) return HG_OK;
  std::lock_guard<std::mutex> g(c->mu);
  return aggregate_host_locked(c, reqs, n, words, nwords, nullptr, codes, agg_pk_out, false);
}

int hg_prepare_aggregate_level(hg_ctx* c, int level) {
  if (!c || level < 0 || level > 2) return HG_ERR_ARG;
  std::lock_guard<std::mutex> g(c->mu);
  return prepare_aggregate_locked(c, level);
}

// ---------------------------------------------------------------- lanes
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
  // exact fold capacities from the requests (what aggregate_host_locked does),
  // and no bitset read outside the staged words
  FoldCaps caps;
  for (size_t i = 0; i < n; i++) {
    const hg_request& r = h_reqs[i];
    if ((size_t)r.word_offset + ((size_t)r.bitlen + 63) / 64 > l->nwords) return HG_ERR_ARG;
    caps.add(r.bitlen);
  }
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
