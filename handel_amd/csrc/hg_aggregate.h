// hg_aggregate.h — the pieces of an aggregate batch (hg_aggregate.cpp) that
// its random-linear-combination form (hg_rlc.cpp) runs as they are: the table
// level and fold workspaces of a submission, the prologue, the fold, the stored
// pairing and its comparison, and the exact path's table-less flow.
#pragma once
#include "hg_ctx.h"

// capacity of a batch's term and chunk lists
struct FoldCaps {
  size_t terms = 0, chunks = 0;
  void add(size_t bitlen);
};
// device-resident requests: their sizes are unknown on the host, every
// request is bounded by the registry
FoldCaps fold_caps_worst(const hg_ctx* c, size_t n);

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

// host-side request validation: the level check of processing.go:350-352
void level_codes(hg_ctx* c, const hg_request* reqs, size_t n, std::vector<int32_t>& out);
// the table level an aggregate submission of n requests runs at (counting
// them towards the volume policy)
int gt_submission_level(hg_ctx* c, size_t n);
int gt_acquire(hg_ctx* c, Ws& ws, hipStream_t s, size_t n, const FoldCaps& caps, int& level, GtWork& w,
               bool may_build = true);
void gt_prologue(hg_ctx* c, const AggBatch& b, Ws& ws, const GtWork& gw, hipStream_t s);
void gt_fold(hg_ctx* c, const AggBatch& b, Ws& ws, const GtWork& gw, int32_t* codes, bool zero_hdr, hipStream_t s);
int pair_stored(hg_ctx* c, const AggBatch& b, Ws& ws, SigForm form, hipStream_t s);
void compare_stored(const AggBatch& b, Ws& ws, const GtWork& gw, hipStream_t s);
int flow_g2_or_mixed(hg_ctx* c, const AggBatch& b, Ws& ws, bool verify, bool use_gt, bool g2_fold, SigForm form,
                     const GtWork& gw, hipStream_t s);
