// hg_ctx.h — the state behind the opaque handles of include/handel_gpu.h
// (hg_ctx, hg_lane, hg_stores) and what every host file of the C ABI shares:
// the submission chain, phase timing, error reporting. Internal: hg_api.cpp
// (context, message, registry, single checks), hg_gttables.cpp (GT tables),
// hg_aggregate.cpp (aggregate verification), hg_lanes.cpp (service lanes),
// hg_rlc.cpp (its random-linear-combination form), hg_intake.cpp (packets,
// stores), hg_pool_api.cpp (the stores' standing queue), hg_msgs.cpp (checks on their own messages), hg_msgs_rlc.cpp (their
// random-linear-combination form) and hg_batch_rlc.cpp (independent checks in
// that form) include it. Every device resource below is held by an owner of
// hg_dev.h, so deleting a context, a lane or a store set frees what it holds.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdlib>
#include <mutex>
#include <string>
#include <utility>
#include <vector>

#include "bn256_gt.h"
#include "bn256_kernels.h"
#include "bn256_mrlc.h"
#include "bn256_rlc.h"
#include "bn256_sigpair.h"
#include "hg_codes.h"
#include "hg_dev.h"
#include "hg_packets.h"
#include "hg_stores.h"

namespace hg {

// Device workspaces of one in-flight submission: the context's own set (every
// hg_* entry point, ordered by the context's submission chain) and one set
// per service lane (hg_lane below), so several lanes' batches run at once
// over the same registry and GT tables.
struct Ws {
  DevBuf<PointG2> pts2;
  DevBuf<PointG1> pts1;
  DevBuf<CheckIn> checks;
  DevBuf<int32_t> codes_b, codes_c;
  DevBuf<int> order;       // aggregation schedule (k_agg_order)
  DevBuf<uint8_t> agg_ws;  // per-request fold results (k_aggregate -> k_agg_finish)
  // GT fold workspaces
  DevBuf<GtReq> gt_plan;
  DevBuf<GtHdr> gt_hdr;
  DevBuf<uint32_t> gt_terms;
  DevBuf<int2> gt_ord;
  DevBuf<int> gt_multi;
  DevBuf<Gt> gt_partial, gt_y;
  // the fold runs on a side stream beside the pairing kernel (GT path): the
  // FE values of the batch land in gt_fe, k_gt_compare joins the two
  Stream side;
  Event ev_fork, ev_join;
  DevBuf<Gt> gt_fe;
  // launch_sig_form's workspace (the 12-lane forms: the batch's lines evaluated
  // at -sig); launch_verify_split (config 2): the Miller values and the final
  // exponentiation's records
  DevBuf<uint8_t> sig_lines;
  // random linear combination (hg_rlc.cpp, bn256_rlc.hip): per check the
  // coefficient and r_i sig_i; per group the live count, the verdict, the G1
  // sum (point and marshal), the 64 subset products and Z_g; the counters; and,
  // grown only when a group fails, the recheck's compact arrays
  DevBuf<uint64_t> rlc_r;
  DevBuf<RlcJac> rlc_jac;
  DevBuf<uint32_t> rlc_glive;
  DevBuf<int32_t> rlc_gcodes;
  DevBuf<PointG1> rlc_gpts;
  DevBuf<uint8_t> rlc_gsigs;
  DevBuf<Gt> rlc_p, rlc_z;
  DevBuf<RlcHdr> rlc_hdr;
  DevBuf<uint32_t> rlc_bcount, rlc_idx;
  DevBuf<uint8_t> rlc_csigs;
  DevBuf<Gt> rlc_cy;
  DevBuf<int32_t> rlc_ccodes;
  size_t rlc_bytes() const {
    return rlc_r.bytes() + rlc_jac.bytes() + rlc_glive.bytes() + rlc_gcodes.bytes() + rlc_gpts.bytes() +
           rlc_gsigs.bytes() + rlc_p.bytes() + rlc_z.bytes() + rlc_hdr.bytes() + rlc_bcount.bytes() + rlc_idx.bytes() +
           rlc_csigs.bytes() + rlc_cy.bytes() + rlc_ccodes.bytes();
  }
  size_t bytes() const {
    return pts2.bytes() + pts1.bytes() + checks.bytes() + codes_b.bytes() + codes_c.bytes() + order.bytes() +
           agg_ws.bytes() + gt_plan.bytes() + gt_hdr.bytes() + gt_terms.bytes() + gt_ord.bytes() + gt_multi.bytes() +
           gt_partial.bytes() + gt_y.bytes() + gt_fe.bytes() + sig_lines.bytes() + rlc_bytes();
  }
};

// Batches whose checks each carry their own message (hg_msgs.cpp): the G1 base
// table (empty until the context's first such call builds it) and the calls'
// workspaces, shared like the others under the context's submission chain.
struct MsgWs {
  DevBuf<PointG1> g1_tab;    // kG1TabEntries: d 16^j G1
  DevBuf<uint32_t> k;        // hashedMessage's scalar, 8 words per check
  DevBuf<int32_t> hcodes;    // HG_OK / HG_ERR_HASH_EOF / HG_ERR_ARG per check
  DevBuf<PointG1> h;         // H per check
  DevBuf<uint8_t> pool;      // the host variants' staging: messages,
  DevBuf<uint32_t> off, len; // their offsets and lengths
  // the combined flow of hg_verify_aggregate_msgs_rlc*, hg_verify_batch_rlc*
  // and hg_verify_batch_msgs_rlc* (MrlcFlow, hg_msgs_rlc.cpp; bn256_msgsrlc.hip):
  // per check r_i k_i mod Order, r_i H_i, the scaled check record and the
  // Miller value; per group its first live member; and, grown only when a
  // group fails, the recheck's compact check records and their H
  DevBuf<uint32_t> rk;
  DevBuf<PointG1> rh;
  DevBuf<CheckIn> rchecks;
  DevBuf<Gt> f;
  DevBuf<uint32_t> carrier;
  DevBuf<CheckIn> cchecks;
  DevBuf<PointG1> ch;
  // the G2 membership verdict of every check's key (bn256_batchrlc.hip), grown
  // only by a flow that asks for it (hg_batch_rlc.cpp) and by hg_debug_g2_member
  DevBuf<uint32_t> member;
  size_t bytes() const {
    return g1_tab.bytes() + k.bytes() + hcodes.bytes() + h.bytes() + pool.bytes() + off.bytes() + len.bytes() +
           rk.bytes() + rh.bytes() + rchecks.bytes() + f.bytes() + carrier.bytes() + cchecks.bytes() + ch.bytes() +
           member.bytes();
  }
};

// The per-message part of the context: hashedMessage and the GT tables
// e(H, .) of the registry. The context keeps the current message's set and
// the previous one (hg_set_message switches between the two without a
// rebuild, so interleaved messages keep their tables).
struct TableSet {
  std::vector<uint8_t> msg;  // the message d_h was hashed from (hg_*_msg cache)
  bool has_msg = false, hash_eof = false;
  DevBuf<PointG1> d_h;  // one point, allocated on the set's first message
  // GT path of aggregate verification (bn256_gttab.hip): e(H, pk_i), window
  // subset products (gt_w8: 8-key windows, gt_win: 16-key windows) and block
  // products, valid for this message and the registry (rebuilt by the first
  // aggregate submission after either changes)
  DevBuf<Gt> gt_key, gt_w8, gt_win, gt_blk;
  // 0: none (aggregates use the G2 fold); 1: e(H, pk_i), 8-key windows and
  // blocks; 2: + 16-key windows. Reset by a message or registry change;
  // raised by hg_prepare_aggregate or by request volume (gt_requests).
  int gt_level = 0;
  // the form of gt_win and gt_blk, meaningful at gt_level 2 (set by every
  // level-2 build): torus form (bn256_gttab.hip), which only k_tor_chunks reads,
  // so a torus set folds over its 16-key windows whatever level a submission
  // asks for; false: Fp12 (the conversion is off, or an entry has no torus form)
  bool torus = false;
  size_t gt_requests = 0;
  size_t table_bytes() const { return gt_key.bytes() + gt_w8.bytes() + gt_win.bytes() + gt_blk.bytes(); }
  // frees the tables (the hash stays); false if the set held none
  bool drop_tables() {
    if (table_bytes() == 0) return false;
    gt_key.reset();
    gt_w8.reset();
    gt_win.reset();
    gt_blk.reset();
    gt_level = 0;
    torus = false;
    return true;
  }
};

}  // namespace hg

using namespace hg;

struct hg_ctx {
  int device = 0;
  int flavor = HG_FLAVOR_GO;
  Stream stream;
  std::mutex mu;
  std::string err;
  // constant tables
  DevBuf<LineCoef> d_lines;
  DevBuf<uint32_t> d_k;
  // the current message's hashedMessage and tables, and the previous
  // message's (set_message_locked swaps the two; see TableSet)
  TableSet cur, alt;
  // registry (nreg > 0 only while every table below matches it)
  DevBuf<PointG2> reg;
  size_t nreg = 0;
  uint64_t reg_gen = 0;  // counts hg_registry_load calls: a hg_stores belongs to one of them
  // aligned block sums of the registry (level k block j at blocks[block_base[k] + j])
  DevBuf<PointG2> blocks;
  // subset sums of every aligned 8-key window (256 per window), the fold's table
  DevBuf<PointG2> wsum;
  std::vector<int> block_base = std::vector<int>(24, 0);
  int block_levels = 0;
  // workspaces
  Ws ws;
  DevBuf<uint8_t> bytes_a, bytes_b;
  DevBuf<PointG1> pts1b;
  DevBuf<int32_t> codes_a;
  DevBuf<hg_request> reqs;
  DevBuf<hg_packet> pkts;  // hg_parse_packets staging
  DevBuf<uint64_t> words;
  MsgWs msgs;  // hg_verify_batch_msgs*, hg_verify_aggregate_msgs*, hg_hash_messages and the combined forms of both
  // -1: the volume policy; 0..2: every aggregate submission at that level
  // (hg_set_aggregate_level; HG_GT_LEVEL / HG_AGG_PATH give the default)
  int pinned_level = -1;
  // highest level this registry may use: lowered when the device (or the
  // table budget) could not hold a level's tables, reset by a registry load
  int gt_cap = 2;
  size_t table_budget = SIZE_MAX;  // bytes of GT tables (hg_set_table_budget)
  // registry keys on the twist but outside G2 (go flavor only: x/crypto's
  // Unmarshal accepts them); any such key pins the registry to level 0. The
  // check (one n*Q per key, ~7 ms of single-lane latency) runs on the side
  // stream after the load; it is waited for only when a GT level is wanted.
  size_t reg_non_g2 = 0;
  bool sub_pending = false;
  Event ev_sub;
  DevBuf<int> sub_count;
  GtBlockIndex gt_bi{};
  // the cap a failed device allocation set (gt_cap also follows the table
  // budget; hg_set_table_budget re-derives gt_cap from this)
  int oom_cap = 2;
  // the context's own aggregate submissions: padded, the two-wave form up to
  // kSigW2MaxN; overlap: hg_set_fold_overlap (HG_GT_OVERLAP=0 gives new contexts false)
  SigPolicy pol;
  // hg_rlc_stats, hg_batch_rlc_stats: the last combined call's (hg_verify_aggregate_rlc*, hg_verify_*_msgs_rlc*,
  // hg_verify_batch_rlc*) groups checked, groups failed, checks re-verified; rlc_read_stats (hg_rlc.cpp) sets them
  uint64_t rlc_stats[3] = {0, 0, 0};
  // hg_batch_rlc_stats: the last hg_verify_batch*_rlc* call's live checks whose key was not proven in G2
  uint64_t brlc_non_g2 = 0;
  bool verify_split = false;  // hg_set_verify_split; HG_VERIFY_SPLIT=1 gives new contexts true
  // submission order across streams: the event recorded after the last
  // submission and the stream it ran on (the workspaces above are shared)
  Event last_ev;
  hipStream_t last_s = nullptr;
  // service lanes (hg_lane): batches in flight on their own workspaces and
  // streams; every context submission first waits for their last batches
  // (they read the registry, H and the tables a submission may rewrite)
  std::vector<hg_lane*> lanes;
  // optional per-phase timing (bench roofline), see hg_timing_read_phase
  bool timing = false;
  std::vector<std::pair<Event, Event>> events[HG_NUM_PHASES];
};

// One service lane (hg_service.cpp): one batch at a time in flight on its own
// stream and workspaces, beside the other lanes' batches. The batch's inputs
// (requests | signatures | bitset words) are staged in pinned host memory and
// go to the device in ONE copy; the codes come back the same way.
struct hg_lane {
  hg_ctx* c = nullptr;
  Ws ws;
  Stream s;
  Event done;
  bool recorded = false;  // `done` marks the lane's last batch
  // hg_lane_set_pairing_padding, hg_lane_set_latency_form, hg_lane_create's overlap
  SigPolicy pol{true, sig_env().w2_lane_max, true};
  Event ev_in;  // hg_lane_submit_device: the caller's stream point
  size_t max_batch = 0, max_words = 0;
  HostBuf<uint8_t> h_in;     // pinned staging
  HostBuf<int32_t> h_codes;  // pinned
  DevBuf<uint8_t> d_in;
  DevBuf<int32_t> d_codes;
  size_t n = 0, nwords = 0, off_sigs = 0, off_words = 0, in_bytes = 0;
  size_t bytes() const { return ws.bytes() + d_in.bytes() + d_codes.bytes(); }
};

// Device-resident stores of the Handel instances a process hosts (hg_stores.hip):
// the tables, the host copy of the receiver map, and the workspaces of the
// host-pointer evaluate and of the selection, sized at creation.
struct hg_stores {
  hg_ctx* c = nullptr;
  uint64_t reg_gen = 0;  // the registry load it was created on
  size_t nreg = 0, max_packets = 0;
  int levels = 0, stride = 0;
  std::vector<uint32_t> receivers;
  std::vector<int32_t> map;  // receiver id -> store index, -1
  DevBuf<uint64_t> tab;
  DevBuf<uint32_t> flags;
  DevBuf<int32_t> d_map;
  // hg_stores_update staging
  DevBuf<hg_store_update> ups;
  DevBuf<uint64_t> up_words;
  // hg_stores_evaluate staging
  DevBuf<hg_packet> pkts;
  DevBuf<uint64_t> words;
  DevBuf<int32_t> codes, scores;
  DevBuf<uint8_t> live;
  // selection
  DevBuf<uint64_t> keys_a, keys_b;
  DevBuf<uint32_t> cnt, picks, base;
  DevBuf<uint8_t> temp;
  // merge (hg_stores_enable_merge; hg_merge.hip): the signature tables, the
  // merge's per-entry workspaces and the staging of the host-pointer calls
  bool merge = false;
  DevBuf<uint8_t> best_sig, indiv_sig;
  DevBuf<uint64_t> held;
  DevBuf<uint32_t> own, m_rows, m_marks;
  DevBuf<hg_store_sig> sig_recs;
  DevBuf<uint8_t> sig_bytes;
  DevBuf<hg_store_query> q_in;
  DevBuf<int32_t> q_codes;
  DevBuf<uint32_t> q_bitlens;
  DevBuf<uint64_t> q_words;
  DevBuf<uint8_t> q_sigs;
  StoreTab table() const {
    return StoreTab{tab.p, flags.p, d_map.p, (uint32_t)nreg, levels, stride, (int)receivers.size()};
  }
  StoreMergeTab merge_table() const { return StoreMergeTab{best_sig.p, indiv_sig.p, held.p, own.p}; }
};

// ---------------------------------------------------------------- submission order
// Every device submission of a context runs between begin() and end(): a
// submission on another stream than the previous one first waits for the
// previous one's event, so two submissions never use the shared workspaces
// (or the registry tables and H) at the same time. Service lanes keep their
// own workspaces; a context submission waits for each lane's last batch.
static inline hipError_t begin(hg_ctx* c, hipStream_t s) {
  if (c->last_ev && c->last_s != s) {
    hipError_t e = hipStreamWaitEvent(s, c->last_ev, 0);
    if (e != hipSuccess) return e;
  }
  for (hg_lane* l : c->lanes) {
    if (!l->recorded) continue;
    hipError_t e = hipStreamWaitEvent(s, l->done, 0);
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}
static inline hipError_t end(hg_ctx* c, hipStream_t s) {
  if (!c->last_ev) {
    hipError_t e = c->last_ev.create(hipEventDisableTiming);
    if (e != hipSuccess) return e;
  }
  c->last_s = s;
  return hipEventRecord(c->last_ev, s);
}
// One submission: end() runs on every exit once start() succeeded, error
// returns included, so a later submission on another stream still waits for
// whatever this one had queued.
struct Submission {
  hg_ctx* c;
  hipStream_t s;
  bool open = false;
  Submission(hg_ctx* c_, hipStream_t s_) : c(c_), s(s_) {}
  hipError_t start() {
    hipError_t e = begin(c, s);
    open = e == hipSuccess;
    return e;
  }
  hipError_t finish() {
    open = false;
    return end(c, s);
  }
  ~Submission() {
    if (open) (void)end(c, s);
  }
};

// ---------------------------------------------------------------- timing
struct PhaseTimer {
  hg_ctx* c;
  int phase;
  hipStream_t s;
  Event a, b;  // an error path that never reaches stop() discards them
  PhaseTimer(hg_ctx* c_, int phase_, hipStream_t s_) : c(c_), phase(phase_), s(s_) {
    if (!c->timing) return;
    if (a.create(hipEventDefault) != hipSuccess || b.create(hipEventDefault) != hipSuccess) {
      a.reset();
      return;
    }
    (void)hipEventRecord(a, s);
  }
  void stop() {
    if (!a) return;
    (void)hipEventRecord(b, s);
    c->events[phase].emplace_back(std::move(a), std::move(b));
  }
};

#define HG_CHECK(ctx, expr)                                                        \
  do {                                                                             \
    hipError_t e_ = (expr);                                                        \
    if (e_ != hipSuccess) {                                                        \
      (ctx)->err = std::string(#expr) + ": " + hipGetErrorString(e_);              \
      return HG_ERR_DEVICE;                                                        \
    }                                                                              \
  } while (0)

static inline int nb(size_t n) { return (int)((n + 255) / 256); }

static inline int check_launch(hg_ctx* c) {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    c->err = std::string("kernel launch: ") + hipGetErrorString(e);
    return HG_ERR_DEVICE;
  }
  return HG_OK;
}

// an integer setting from the environment; `def` when unset or outside [lo, hi]
static inline int env_int(const char* name, int def, int lo, int hi) {
  const char* e = getenv(name);
  const int v = e ? atoi(e) : def;
  return v >= lo && v <= hi ? v : def;
}
// the side stream of a workspace set and its fork/join events, on first use
static inline hipError_t ensure_side(Ws& ws) {
  hipError_t e = hipSuccess;
  if (!ws.side) e = ws.side.create(hipStreamNonBlocking);
  if (e == hipSuccess && !ws.ev_fork) e = ws.ev_fork.create(hipEventDisableTiming);
  if (e == hipSuccess && !ws.ev_join) e = ws.ev_join.create(hipEventDisableTiming);
  return e;
}

// hg_api.cpp: hashedMessage of `msg` as the current message (c->mu held)
int set_message_locked(hg_ctx* c, const uint8_t* msg, size_t len);
// what HG_GT_LEVEL / HG_AGG_PATH (hg_gttables.cpp) and HG_GT_OVERLAP (hg_aggregate.cpp) give new contexts
int gt_forced_level();
bool gt_overlap();
