// hg_aggregate.h — the internal interface of aggregate verification: what
// hg_gttables.cpp (the GT tables), hg_aggregate.cpp (a batch's workspaces, flows,
// staging and entry points), hg_lanes.cpp (the service lanes), hg_rlc.cpp (the
// random-linear-combination form), hg_msgs.cpp (a message per request),
// hg_msgs_rlc.cpp (its combined form) and hg_batch_rlc.cpp (independent checks
// in that form) use of each other. Every name below has users in at least two of them.
#pragma once
#include <optional>

#include "hg_ctx.h"

// internal return code: an allocation of the GT path failed (the caller falls back to a lower level)
static constexpr int kNoMem = -1;
// an allocation of the GT path: out of device memory -> kNoMem, any other failure -> HG_ERR_DEVICE
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

// ---------------------------------------------------------------- hg_gttables.cpp
// the table level an aggregate submission of n requests runs at (counting them towards the volume policy)
int gt_submission_level(hg_ctx* c, size_t n);
// builds up to `level` on stream s, lowering it (and the context's cap) to what the device and the budget hold
int build_fitting_locked(hg_ctx* c, hipStream_t s, int& level);
// the registry's G2 membership count into c->reg_non_g2, waiting for its check if still running
int resolve_subgroup(hg_ctx* c);

// ---------------------------------------------------------------- hg_aggregate.cpp
// capacity of a batch's term and chunk lists
struct FoldCaps {
  size_t terms = 0, chunks = 0;
  void add(size_t bitlen);
};
// device-resident requests: their sizes are unknown on the host, every request is bounded by the registry
FoldCaps fold_caps_worst(const hg_ctx* c, size_t n);
// terms per fold chunk (HG_GT_CHUNK)
int gt_chunk();

// The parts of a workspace set a batch of n requests needs, sized in one place
// for a submission and for a lane (every part it may ever use at its largest
// batch: a buffer that grew later would be freed and reallocated between
// batches, and freeing device memory waits for the whole device). Verify: the
// decoded signatures and their codes; Level: level codes computed here; G2Fold,
// GtFold (caps): the folds'; AggOut: the aggregate keys; Pairing: the FE values
// and launch_sig_form's sig_bytes; Side: the side stream and its events.
enum : unsigned { kWsVerify = 1, kWsLevel = 2, kWsG2Fold = 4, kWsAggOut = 8, kWsGtFold = 16, kWsPairing = 32, kWsSide = 64 };
hipError_t ws_ensure(Ws& ws, size_t n, unsigned parts, const FoldCaps& caps = {}, size_t sig_bytes = 0);

// One batch on the device: n requests, their bitset words and signatures in;
// codes (and, nullable, agg: the aggregate keys' marshals; bits: the verdict
// bitset of the codes, hg_pack_verdicts_device's layout) out. lvl (nullable):
// the level codes, updated in place; computed here when the flow needs them.
// caps (nullable): the fold's list capacities; else bounded by the registry.
struct AggBatch {
  const hg_request* reqs;
  size_t n;
  const uint64_t* words;
  const uint8_t* sigs;
  int32_t* codes;
  uint8_t* agg = nullptr;
  int32_t* lvl = nullptr;
  uint8_t* bits = nullptr;
  const FoldCaps* caps = nullptr;
};

// The table level of one submission (inside it, on stream s) and its fold work:
// the policy's level, the tables and fold workspaces it needs (may_build = false:
// a lane runs at the built level at most), the torus rule, gw's win_bits and torus.
int submission_level(hg_ctx* c, const AggBatch& b, Ws& ws, hipStream_t s, bool may_build, int& level, GtWork& gw);
// the GT flows' first launch: level check, signature decode, the fold's counters
void gt_prologue(hg_ctx* c, const AggBatch& b, Ws& ws, const GtWork& gw, hipStream_t s);
// the GT fold of the batch into ws.gt_y (codes: in and out)
void gt_fold(hg_ctx* c, const AggBatch& b, Ws& ws, const GtWork& gw, int32_t* codes, bool zero_hdr, hipStream_t s);
// the pairing in its stored form: ws.gt_fe[r] = FE(Miller(G2Base at -sig_r))
int pair_stored(hg_ctx* c, const AggBatch& b, Ws& ws, SigForm form, hipStream_t s);
// the stored FE values against ws.gt_y
void compare_stored(const AggBatch& b, Ws& ws, const GtWork& gw, hipStream_t s);
// the G2 fold, the GT fold beside it when use_gt, and (verify) the check
int flow_g2_or_mixed(hg_ctx* c, const AggBatch& b, Ws& ws, bool verify, bool use_gt, bool g2_fold, SigForm form,
                     const GtWork& gw, hipStream_t s);
// the Combine fold and (verify) the pairing check of a batch on stream s with the workspaces ws (is_lane: a lane's)
int aggregate_device_locked(hg_ctx* c, const AggBatch& b, bool verify, hipStream_t s, Ws& ws, const SigPolicy& pol,
                            bool is_lane);

// A host-pointer aggregate batch as its entry point received it (who: its name, for hg_last_error).
struct HostBatch {
  const char* who;
  const hg_request* reqs;
  size_t n;
  const uint64_t* words;
  size_t nwords;
  const uint8_t* sigs;  // nullable: hg_aggregate_pk has none
};
// the host entry points' request check (hg_requests.h, level errors skipped): HG_ERR_ARG with the request named
// in hg_last_error; lvl (nullable): the level codes; caps (nullable): the fold's exact capacities
int check_host_requests(hg_ctx* c, const HostBatch& h, int32_t* lvl, FoldCaps* caps);
// The staging of a host-pointer batch on the context's stream, inside one
// submission: open() grows the context's staging buffers and uploads requests,
// words and signatures, put() uploads one more array, close() copies the codes
// (and the aggregate keys) back and synchronises.
struct HostStage {
  hg_ctx* c;
  Submission sub;
  uint8_t* d_keys = nullptr;  // the aggregate keys' marshals on the device, when open() was asked for them
  explicit HostStage(hg_ctx* c_) : c(c_), sub(c_, c_->stream) {}
  int open(const HostBatch& h, bool want_keys);
  template <class T>
  int put(DevBuf<T>& dst, const void* src, size_t count) {
    HG_CHECK(c, dst.ensure(count));
    HG_CHECK(c, hipMemcpyAsync(dst.p, src, count * sizeof(T), hipMemcpyHostToDevice, c->stream));
    return HG_OK;
  }
  // the staged batch: codes in c->codes_a, keys in d_keys
  AggBatch batch(const HostBatch& h) const {
    return AggBatch{c->reqs.p, h.n, c->words.p, h.sigs ? c->bytes_b.p : nullptr, c->codes_a.p, d_keys};
  }
  int close(const HostBatch& h, const int32_t* d_codes, int32_t* codes, uint8_t* keys_out);
};
// VerifyMultiSignature's requests: the range [0, N) with the multisignature's own bit count
std::vector<hg_request> multisig_requests(const hg_ctx* c, const uint32_t* bitlens, const uint32_t* word_offsets,
                                          size_t n);

// ---------------------------------------------------------------- hg_rlc.cpp
// One combined call as its entry point asked for it (who: its name, for hg_last_error).
struct RlcCall {
  const char* who;
  const uint8_t* seed;       // 32 bytes, or
  const uint64_t* d_coeffs;  // the probes' coefficients (device)
  uint32_t group;
  bool recheck;  // false: a probe stops after the group verdicts
};
// hg_rlc_stats of a call that did not run the combination
void rlc_clear_stats(hg_ctx* c);
// The one read-back of a combined call: ws.rlc_hdr to *h on stream s, synchronised,
// into c->rlc_stats; HG_ERR_DEVICE if it counts more failed members than the n checks.
int rlc_read_stats(hg_ctx* c, const RlcCall& call, size_t n, hipStream_t s, RlcHdr* h);
// the probes' copy-out of the ng groups' verdicts and live counts (stream s, not synchronised)
int rlc_copy_groups(hg_ctx* c, size_t ng, int32_t* group_codes, uint32_t* group_live, hipStream_t s);

// ---------------------------------------------------------------- hg_msgs.cpp
// the G1 base table of launch_hash_points, built on stream s by the context's first call that needs it
int ensure_g1_table(hg_ctx* c, hipStream_t s);
// the host variants' argument check: every message range inside the pool (HG_ERR_ARG, the message named)
int check_ranges(hg_ctx* c, const char* who, size_t pool_len, const uint32_t* off, const uint32_t* len, size_t n);
// pool, offsets and lengths into c->msgs (c->stream, inside the caller's submission)
int stage_messages(hg_ctx* c, const uint8_t* pool, size_t pool_len, const uint32_t* off, const uint32_t* len,
                   size_t n);
// hg_verify_aggregate_msgs_device's batch on stream s: the exact path (d_agg nullable)
int aggregate_msgs_device_locked(hg_ctx* c, const uint8_t* d_pool, size_t pool_len, const uint32_t* d_off,
                                 const uint32_t* d_len, const hg_request* d_reqs, size_t n, const uint64_t* d_words,
                                 const uint8_t* d_sigs, int32_t* d_codes, uint8_t* d_agg, hipStream_t s);

// ---------------------------------------------------------------- hg_msgs_rlc.cpp
// The combined flow of n checks that carry a message each, on stream s with
// the context's workspaces: this file's requests and hg_batch_rlc.cpp's
// independent checks. hs is the side stream, or s with hg_set_fold_overlap(ctx, 0).
//   s:  coefficients -> the caller's check records and codes ..... -> wait -> the caller's code merge -> G1 sums,
//       scaled records, Miller loops, group products, FE, verdicts (members: G2 membership) (-> recheck)
//   hs: wait -> the caller's H per check, k_mrlc_scalars, k_hash_points (r H) -> join
// A caller runs, returning the first error as it stands:
//   mrlc_begin;  on f.hs its H per check into c->msgs.k, hcodes and h;  mrlc_hashed;
//   on s its check records into c->ws.checks and their codes;  mrlc_wait_hashed;
//   on s its merge of c->msgs.hcodes into the codes;  mrlc_finish.
struct MrlcFlow {
  hg_ctx* c;
  const RlcCall& call;
  size_t n;
  bool members;  // the Miller kernel also yields the G2 membership of every check's key (c->msgs.member)
  hipStream_t s;
  hipStream_t hs = nullptr;  // from mrlc_begin on
  RlcHdr hdr{};              // the call's counters once mrlc_finish read them back (call.recheck)
  Submission sub;
  std::optional<PhaseTimer> all;  // HG_PHASE_SUBMIT, from the submission's start to mrlc_finish
  MrlcFlow(hg_ctx* c_, const RlcCall& call_, size_t n_, bool members_, hipStream_t s_)
      : c(c_), call(call_), n(n_), members(members_), s(s_), sub(c_, s_) {}
  size_t ng() const { return rlc_groups(n, call.group); }
};
// grows the workspaces, starts the submission, draws the coefficients, forks hs and builds the G1 table there
int mrlc_begin(MrlcFlow& f);
// after the caller's H per check: r_i H_i and the join record
int mrlc_hashed(MrlcFlow& f);
// s waits for the join
int mrlc_wait_hashed(MrlcFlow& f);
// the combination over c->ws.checks and codes, the recheck of the failed groups' live members, the submission's end
int mrlc_finish(MrlcFlow& f, int32_t* codes);
