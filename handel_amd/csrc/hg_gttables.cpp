// hg_gttables.cpp — the GT tables of aggregate verification behind
// include/handel_gpu.h: the policy that picks a context's table level, the
// builds (hg_prepare_aggregate*, and build_fitting_locked inside a submission
// of hg_aggregate.cpp), the table budget and the calls that report on them.
#include <cstring>

#include "hg_aggregate.h"

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
int resolve_subgroup(hg_ctx* c) {
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
int build_fitting_locked(hg_ctx* c, hipStream_t s, int& level) {
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

int hg_prepare_aggregate_level(hg_ctx* c, int level) {
  if (!c || level < 0 || level > 2) return HG_ERR_ARG;
  std::lock_guard<std::mutex> g(c->mu);
  return prepare_aggregate_locked(c, level);
}

// The current message's table set as built (the value-level tests read it back)
int hg_debug_gt_layout(hg_ctx* c, int32_t* out) {
  if (!c || !out) return HG_ERR_ARG;
  std::lock_guard<std::mutex> g(c->mu);
  if (c->cur.gt_level < 1 || c->nreg == 0) {
    c->err = "hg_debug_gt_layout: no tables are built";
    return HG_ERR_ARG;
  }
  int cnt[24] = {0};
  gt_block_count(c, cnt);
  memset(out, 0, HG_GT_LAYOUT_WORDS * sizeof(int32_t));
  out[0] = c->cur.gt_level;
  out[1] = c->cur.gt_level == 2 && c->cur.torus ? 1 : 0;
  out[2] = (int32_t)c->nreg;
  out[3] = (int32_t)((c->nreg + 7) / 8);
  out[4] = (int32_t)((c->nreg + 15) / 16);
  out[5] = c->block_levels < 23 ? c->block_levels : 23;
  for (int k = 4; k <= out[5]; k++) {
    out[6 + k] = c->gt_bi.base[k];
    out[30 + k] = cnt[k];
  }
  return HG_OK;
}

int hg_debug_gt_entries(hg_ctx* c, int table, size_t first, size_t count, uint32_t* out) {
  if (!c || !out) return HG_ERR_ARG;
  std::lock_guard<std::mutex> g(c->mu);
  const Gt* src = nullptr;
  size_t have = 0;
  if (c->cur.gt_level >= 1 && c->nreg > 0) {
    if (table == HG_GT_TABLE_KEYS) src = c->cur.gt_key.p, have = c->nreg;
    else if (table == HG_GT_TABLE_WIN8) src = c->cur.gt_w8.p, have = (c->nreg + 7) / 8 * 256;
    else if (table == HG_GT_TABLE_BLOCKS) src = c->cur.gt_blk.p, have = gt_block_count(c, nullptr);
    else if (table == HG_GT_TABLE_WIN16 && c->cur.gt_level >= 2) src = c->cur.gt_win.p, have = (c->nreg + 15) / 16 * 65536;
  }
  if (!src || first > have || count > have - first) {
    c->err = "hg_debug_gt_entries: no such table is built, or the range leaves it";
    return HG_ERR_ARG;
  }
  if (count == 0) return HG_OK;
  HG_CHECK(c, hipSetDevice(c->device));
  // every build is synchronous or inside a submission this one is ordered after
  Submission sub(c, c->stream);
  HG_CHECK(c, sub.start());
  HG_CHECK(c, hipMemcpyAsync(out, src + first, count * sizeof(Gt), hipMemcpyDeviceToHost, c->stream));
  HG_CHECK(c, sub.finish());
  HG_CHECK(c, hipStreamSynchronize(c->stream));
  return HG_OK;
}

}  // extern "C"
