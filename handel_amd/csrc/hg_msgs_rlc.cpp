// hg_msgs_rlc.cpp — hg_verify_aggregate_msgs_rlc*, hg_verify_multisig_msgs_rlc
// and their two probes behind include/handel_gpu.h: aggregate requests that
// each carry their own message (VerifyMultiSignature(msg, ...), crypto.go:120-137;
// verifySignature, processing.go:342-368) with one final exponentiation per
// group of requests (bn256_msgsrlc.hip). A batch runs the exact
// call's fold, hash and code merge (hg_msgs.cpp), then per request one Miller
// loop on r_i H_i and per group one Fp12 product, one final exponentiation and
// the verdict; the live members of a group that fails go through the exact
// call's two-pairing check (k_msgs_verify). A registry that is not proven in G2
// runs the exact call as it stands.
#include <cstring>

#include "bn256_sigform.h"
#include "hg_aggregate.h"

namespace {

struct MrlcCall {
  const char* who;
  const uint8_t* seed;       // 32 bytes, or
  const uint64_t* d_coeffs;  // the probe's coefficients (device)
  uint32_t group;
  bool recheck;  // false: hg_debug_msgs_rlc_groups stops after the group verdicts
};

// the batch's messages and requests on the device
struct MsgBatch {
  const uint8_t* pool;
  size_t pool_len;
  const uint32_t *off, *len;
  const hg_request* reqs;
  size_t n;
  const uint64_t* words;
  const uint8_t* sigs;
  int32_t* codes;
};

RlcSeed seed_of(const uint8_t* seed) {
  RlcSeed sd{};
  if (seed) memcpy(sd.b, seed, 32);
  return sd;
}

hipError_t mrlc_ensure(hg_ctx* c, size_t n, size_t ng) {
  Ws& ws = c->ws;
  MsgWs& mw = c->msgs;
  hipError_t e = hipSuccess;
  auto grow = [&e](auto& buf, size_t count) {
    if (e == hipSuccess) e = buf.ensure(count);
  };
  // the exact flow's
  grow(ws.checks, n), grow(ws.order, n), grow(ws.agg_ws, n * agg_partial_bytes() + agg_fixed_bytes());
  grow(ws.codes_c, n), grow(mw.k, 8 * n), grow(mw.hcodes, n), grow(mw.h, n);
  // the combination's
  grow(ws.pts1, n), grow(ws.rlc_r, n), grow(ws.rlc_jac, n);
  grow(ws.rlc_glive, ng), grow(ws.rlc_gcodes, ng), grow(ws.rlc_gpts, ng), grow(ws.rlc_z, ng), grow(ws.rlc_hdr, 1);
  grow(ws.sig_lines, fe12_ws_bytes((int)ng));
  grow(mw.rk, 8 * n), grow(mw.rh, n), grow(mw.rchecks, n), grow(mw.f, n), grow(mw.carrier, ng);
  return e;
}

// The failed groups' live members through the exact check: gathered in index
// order with their unscaled H, verified as a batch of their own, the codes
// scattered back.
int mrlc_recheck(hg_ctx* c, const MsgBatch& b, uint32_t group, size_t m, hipStream_t s) {
  Ws& ws = c->ws;
  MsgWs& mw = c->msgs;
  HG_CHECK(c, ws.rlc_bcount.ensure((b.n + 255) / 256));
  HG_CHECK(c, ws.rlc_idx.ensure(m));
  HG_CHECK(c, ws.rlc_ccodes.ensure(m));
  HG_CHECK(c, mw.cchecks.ensure(m));
  HG_CHECK(c, mw.ch.ensure(m));
  launch_mrlc_gather(b.codes, ws.rlc_gcodes.p, (int)b.n, group, ws.checks.p, mw.h.p, ws.rlc_bcount.p, ws.rlc_idx.p,
                     mw.cchecks.p, mw.ch.p, ws.rlc_ccodes.p, s);
  launch_verify_msgs(mw.cchecks.p, (int)m, c->d_lines.p, mw.ch.p, ws.rlc_ccodes.p, s);
  launch_rlc_scatter(ws.rlc_idx.p, ws.rlc_ccodes.p, (int)m, b.codes, s);
  return HG_OK;
}

// One batch on stream s with the context's workspaces. *ran: the combination
// ran (false: the exact call did).
//   s:    coefficients -> level codes, G2 fold ............ -> wait -> merge -> G1 sums, scaled records,
//                                                             k_mrlc_miller, k_mrlc_product, FE, verdicts (-> recheck)
//   side: wait -> k_hash_scalars, k_hash_points (H), k_mrlc_scalars, k_hash_points (r H) -> join
int mrlc_device_locked(hg_ctx* c, const MsgBatch& b, const MrlcCall& call, bool* ran, hipStream_t s) {
  *ran = false;
  c->rlc_stats[0] = c->rlc_stats[1] = c->rlc_stats[2] = 0;
  if (c->nreg == 0) {
    c->err = std::string(call.who) + ": needs a registry";
    return HG_ERR_ARG;
  }
  const size_t n = b.n, ng = (n + call.group - 1) / call.group;
  // Every D_i = e(H_i, agg_i) e(-sig_i, G2Base) must lie in the order-n
  // subgroup: aggregates of a registry proven in G2 do (G1 has cofactor 1).
  int rc = resolve_subgroup(c);
  if (rc) return rc;
  if (c->reg_non_g2 || n > (size_t)kSig12MaxN) {
    if (!call.recheck) {
      c->err = std::string(call.who) + ": the context would not run the combination";
      return HG_ERR_ARG;
    }
    return aggregate_msgs_device_locked(c, b.pool, b.pool_len, b.off, b.len, b.reqs, n, b.words, b.sigs, b.codes,
                                        nullptr, s);
  }
  Ws& ws = c->ws;
  MsgWs& mw = c->msgs;
  const bool beside = c->pol.overlap;
  HG_CHECK(c, mrlc_ensure(c, n, ng));
  if (beside) HG_CHECK(c, ensure_side(ws));
  Submission sub(c, s);
  HG_CHECK(c, sub.start());
  PhaseTimer all(c, HG_PHASE_SUBMIT, s);
  launch_rlc_prep(seed_of(call.seed), call.d_coeffs, (int)n, (int)ng, ws.rlc_r.p, ws.rlc_gcodes.p, ws.rlc_hdr.p, s);
  const hipStream_t hs = beside ? ws.side.h : s;
  if (beside) {
    HG_CHECK(c, hipEventRecord(ws.ev_fork, s));
    HG_CHECK(c, hipStreamWaitEvent(hs, ws.ev_fork, 0));
  }
  rc = ensure_g1_table(c, hs);
  if (rc == HG_OK) {
    // H_i for the recheck and r_i H_i for the combination: two walks of the
    // fixed-base table, no G1 chain and no inversion more than that
    launch_hash_scalars(b.pool, b.pool_len, b.off, b.len, (int)n, mw.k.p, mw.hcodes.p, hs);
    launch_hash_points(mw.k.p, mw.hcodes.p, (int)n, mw.g1_tab.p, mw.h.p, hs);
    launch_mrlc_scalars(mw.k.p, mw.hcodes.p, ws.rlc_r.p, (int)n, mw.rk.p, hs);
    launch_hash_points(mw.rk.p, mw.hcodes.p, (int)n, mw.g1_tab.p, mw.rh.p, hs);
    rc = check_launch(c);
  }
  if (beside) HG_CHECK(c, hipEventRecord(ws.ev_join, hs));
  if (rc) {
    if (beside) (void)hipStreamWaitEvent(s, ws.ev_join, 0);  // the submission's end covers the side stream
    return rc;
  }
  launch_aggmsgs_levels(b.reqs, (int)n, (uint32_t)c->nreg, ws.codes_c.p, s);
  PhaseTimer fold(c, HG_PHASE_AGGREGATE, s);
  launch_aggregate(c->wsum.p, (int)c->nreg, c->blocks.p, c->block_base.data(), c->block_levels, b.reqs, (int)n, b.words,
                   ws.order.p, ws.agg_ws.p, ws.checks.p, ws.codes_c.p, s);
  fold.stop();
  if (beside) HG_CHECK(c, hipStreamWaitEvent(s, ws.ev_join, 0));
  launch_aggmsgs_merge(b.sigs, (int)n, c->flavor, ws.codes_c.p, mw.hcodes.p, ws.checks.p, b.codes, s);
  PhaseTimer t(c, HG_PHASE_VERIFY, s);
  // sum r_i sig_i per group over the live members
  launch_mrlc_sigs(ws.checks.p, (int)n, ws.pts1.p, s);
  launch_rlc_g1_mul(ws.pts1.p, b.codes, ws.rlc_r.p, (int)n, ws.rlc_jac.p, s);
  launch_rlc_g1_sum(ws.rlc_jac.p, b.codes, (int)n, call.group, (int)ng, ws.rlc_gpts.p, ws.rlc_glive.p, s);
  launch_mrlc_checks(ws.checks.p, b.codes, ws.rlc_gpts.p, (int)n, call.group, (int)ng, mw.carrier.p, mw.rchecks.p, s);
  launch_mrlc_miller(mw.rchecks.p, (int)n, c->d_lines.p, mw.rh.p, mw.f.p, s);
  launch_mrlc_product(mw.f.p, b.codes, (int)n, call.group, (int)ng, ws.rlc_z.p, s);
  if (!launch_fe12(ws.rlc_z.p, (int)ng, ws.sig_lines.p, s)) {
    c->err = std::string(call.who) + ": too many groups for the final exponentiation";
    return HG_ERR_ARG;
  }
  launch_fe_verdicts(ws.rlc_z.p, (int)ng, ws.rlc_gcodes.p, s);
  launch_rlc_count(ws.rlc_gcodes.p, ws.rlc_glive.p, (int)ng, ws.rlc_hdr.p, s);
  rc = check_launch(c);
  if (rc) return rc;
  *ran = true;
  if (call.recheck) {
    // the one read-back: how many requests the failed groups hold sizes their launch
    RlcHdr h{};
    HG_CHECK(c, hipMemcpyAsync(&h, ws.rlc_hdr.p, sizeof h, hipMemcpyDeviceToHost, s));
    HG_CHECK(c, hipStreamSynchronize(s));
    c->rlc_stats[0] = h.groups;
    c->rlc_stats[1] = h.groups_failed;
    c->rlc_stats[2] = h.failed_members;
    if (h.failed_members > n) {
      c->err = std::string(call.who) + ": inconsistent failed-member count";
      return HG_ERR_DEVICE;
    }
    if (h.failed_members) {
      rc = mrlc_recheck(c, b, call.group, h.failed_members, s);
      if (rc) return rc;
    }
  }
  t.stop();
  all.stop();
  rc = check_launch(c);
  if (rc) return rc;
  HG_CHECK(c, sub.finish());
  return HG_OK;
}

// host pointers in, through the context's staging buffers (as hg_verify_aggregate_msgs)
int mrlc_host_locked(hg_ctx* c, const uint8_t* pool, size_t pool_len, const uint32_t* off, const uint32_t* len,
                     const HostBatch& h, const uint64_t* coeffs, const MrlcCall& call0, int32_t* codes,
                     int32_t* group_codes, uint32_t* group_live) {
  const size_t n = h.n;
  int rc = check_ranges(c, h.who, pool_len, off, len, n);
  if (rc) return rc;
  if (c->nreg == 0) {
    c->err = std::string(h.who) + ": needs a registry";
    return HG_ERR_ARG;
  }
  rc = check_host_requests(c, h, nullptr, nullptr);
  if (rc) return rc;
  HostStage st(c);
  rc = st.open(h, false);
  if (rc == HG_OK) rc = stage_messages(c, pool, pool_len, off, len, n);
  if (rc == HG_OK && coeffs) rc = st.put(c->bytes_a, coeffs, n * 8);
  if (rc) return rc;
  MrlcCall call = call0;
  call.d_coeffs = coeffs ? reinterpret_cast<const uint64_t*>(c->bytes_a.p) : nullptr;
  const AggBatch ab = st.batch(h);
  const MsgBatch b{c->msgs.pool.p, pool_len, c->msgs.off.p, c->msgs.len.p, ab.reqs, n, ab.words, ab.sigs, ab.codes};
  bool ran = false;
  rc = mrlc_device_locked(c, b, call, &ran, c->stream);
  if (rc) return rc;
  if (group_codes && ran) {
    const size_t ng = (n + call.group - 1) / call.group;
    HG_CHECK(c, hipMemcpyAsync(group_codes, c->ws.rlc_gcodes.p, ng * 4, hipMemcpyDeviceToHost, c->stream));
    HG_CHECK(c, hipMemcpyAsync(group_live, c->ws.rlc_glive.p, ng * 4, hipMemcpyDeviceToHost, c->stream));
  }
  return st.close(h, b.codes, codes, nullptr);
}

bool group_ok(uint32_t group) { return group >= 1 && group <= kRlcMaxGroup; }

}  // namespace

extern "C" {

int hg_verify_aggregate_msgs_rlc(hg_ctx* c, const uint8_t* pool, size_t pool_len, const uint32_t* msg_off,
                                 const uint32_t* msg_len, const hg_request* reqs, size_t n, const uint64_t* words,
                                 size_t nwords, const uint8_t* sigs, const uint8_t seed[32], uint32_t group,
                                 int32_t* codes) {
  if (!c || !seed || !group_ok(group) || (n && (!msg_off || !msg_len || !reqs || !sigs || !codes)) ||
      (!pool && pool_len) || (!words && nwords) || n > (size_t)INT32_MAX)
    return HG_ERR_ARG;
  std::lock_guard<std::mutex> g(c->mu);
  c->rlc_stats[0] = c->rlc_stats[1] = c->rlc_stats[2] = 0;
  if (n == 0) return HG_OK;
  return mrlc_host_locked(c, pool, pool_len, msg_off, msg_len,
                          HostBatch{"hg_verify_aggregate_msgs_rlc", reqs, n, words, nwords, sigs}, nullptr,
                          MrlcCall{"hg_verify_aggregate_msgs_rlc", seed, nullptr, group, true}, codes, nullptr, nullptr);
}

int hg_verify_aggregate_msgs_rlc_device(hg_ctx* c, const uint8_t* d_pool, size_t pool_len, const uint32_t* d_msg_off,
                                        const uint32_t* d_msg_len, const hg_request* d_reqs, size_t n,
                                        const uint64_t* d_words, const uint8_t* d_sigs, const uint8_t seed[32],
                                        uint32_t group, int32_t* d_codes, void* stream) {
  if (!c || !seed || !group_ok(group) || (n && (!d_msg_off || !d_msg_len || !d_reqs || !d_sigs || !d_codes)) ||
      (!d_pool && pool_len) || n > (size_t)INT32_MAX)
    return HG_ERR_ARG;
  std::lock_guard<std::mutex> g(c->mu);
  c->rlc_stats[0] = c->rlc_stats[1] = c->rlc_stats[2] = 0;
  if (n == 0) return HG_OK;
  HG_CHECK(c, hipSetDevice(c->device));
  hipStream_t s = stream ? (hipStream_t)stream : c->stream;
  bool ran = false;
  return mrlc_device_locked(c, MsgBatch{d_pool, pool_len, d_msg_off, d_msg_len, d_reqs, n, d_words, d_sigs, d_codes},
                            MrlcCall{"hg_verify_aggregate_msgs_rlc_device", seed, nullptr, group, true}, &ran, s);
}

int hg_verify_multisig_msgs_rlc(hg_ctx* c, const uint8_t* pool, size_t pool_len, const uint32_t* msg_off,
                                const uint32_t* msg_len, const uint32_t* bitlens, const uint32_t* word_offsets,
                                size_t n, const uint64_t* words, size_t nwords, const uint8_t* sigs,
                                const uint8_t seed[32], uint32_t group, int32_t* codes) {
  if (!c || !seed || !group_ok(group) ||
      (n && (!msg_off || !msg_len || !bitlens || !word_offsets || !sigs || !codes)) || (!pool && pool_len) ||
      (!words && nwords) || n > (size_t)INT32_MAX)
    return HG_ERR_ARG;
  std::lock_guard<std::mutex> g(c->mu);
  c->rlc_stats[0] = c->rlc_stats[1] = c->rlc_stats[2] = 0;
  if (n == 0) return HG_OK;
  // crypto.go:121-124: the bitset must span the registry (bitlen != N is the
  // level error of the request [0, N), renamed on the host); the rest is verifySignature
  const std::vector<hg_request> reqs = multisig_requests(c, bitlens, word_offsets, n);
  int rc = mrlc_host_locked(c, pool, pool_len, msg_off, msg_len,
                            HostBatch{"hg_verify_multisig_msgs_rlc", reqs.data(), n, words, nwords, sigs}, nullptr,
                            MrlcCall{"hg_verify_multisig_msgs_rlc", seed, nullptr, group, true}, codes, nullptr,
                            nullptr);
  if (rc) return rc;
  for (size_t i = 0; i < n; i++)
    if (codes[i] == HG_ERR_LEVEL) codes[i] = HG_ERR_MULTI_SIZES;
  return HG_OK;
}

int hg_debug_msgs_rlc_groups(hg_ctx* c, const uint8_t* pool, size_t pool_len, const uint32_t* msg_off,
                             const uint32_t* msg_len, const hg_request* reqs, size_t n, const uint64_t* words,
                             size_t nwords, const uint8_t* sigs, const uint64_t* coeffs, uint32_t group,
                             int32_t* codes, int32_t* group_codes, uint32_t* group_live) {
  if (!c || !group_ok(group) ||
      (n && (!msg_off || !msg_len || !reqs || !sigs || !coeffs || !codes || !group_codes || !group_live)) ||
      (!pool && pool_len) || (!words && nwords) || n > (size_t)INT32_MAX)
    return HG_ERR_ARG;
  if (n == 0) return HG_OK;
  std::lock_guard<std::mutex> g(c->mu);
  return mrlc_host_locked(c, pool, pool_len, msg_off, msg_len,
                          HostBatch{"hg_debug_msgs_rlc_groups", reqs, n, words, nwords, sigs}, coeffs,
                          MrlcCall{"hg_debug_msgs_rlc_groups", nullptr, nullptr, group, false}, codes, group_codes,
                          group_live);
}

int hg_debug_msgs_rlc_points(hg_ctx* c, const uint8_t* pool, size_t pool_len, const uint32_t* msg_off,
                             const uint32_t* msg_len, const uint64_t* coeffs, size_t n, uint8_t* out) {
  if (!c || (n && (!msg_off || !msg_len || !coeffs || !out)) || (!pool && pool_len) || n > (size_t)INT32_MAX)
    return HG_ERR_ARG;
  if (n == 0) return HG_OK;
  std::lock_guard<std::mutex> g(c->mu);
  int rc = check_ranges(c, "hg_debug_msgs_rlc_points", pool_len, msg_off, msg_len, n);
  if (rc) return rc;
  HG_CHECK(c, hipSetDevice(c->device));
  Ws& ws = c->ws;
  MsgWs& mw = c->msgs;
  hipStream_t s = c->stream;
  HG_CHECK(c, c->bytes_a.ensure(n * 64));
  HG_CHECK(c, ws.rlc_r.ensure(n));
  HG_CHECK(c, mw.k.ensure(8 * n));
  HG_CHECK(c, mw.hcodes.ensure(n));
  HG_CHECK(c, mw.rk.ensure(8 * n));
  HG_CHECK(c, mw.rh.ensure(n));
  Submission sub(c, s);
  HG_CHECK(c, sub.start());
  rc = stage_messages(c, pool, pool_len, msg_off, msg_len, n);
  if (rc == HG_OK) rc = ensure_g1_table(c, s);
  if (rc) return rc;
  HG_CHECK(c, hipMemcpyAsync(ws.rlc_r.p, coeffs, n * 8, hipMemcpyHostToDevice, s));
  launch_hash_scalars(mw.pool.p, pool_len, mw.off.p, mw.len.p, (int)n, mw.k.p, mw.hcodes.p, s);
  launch_mrlc_scalars(mw.k.p, mw.hcodes.p, ws.rlc_r.p, (int)n, mw.rk.p, s);
  launch_hash_points(mw.rk.p, mw.hcodes.p, (int)n, mw.g1_tab.p, mw.rh.p, s);
  launch_encode_g1(mw.rh.p, (int)n, c->bytes_a.p, s);
  rc = check_launch(c);
  if (rc) return rc;
  std::vector<int32_t> hcodes(n);
  HG_CHECK(c, hipMemcpyAsync(out, c->bytes_a.p, n * 64, hipMemcpyDeviceToHost, s));
  HG_CHECK(c, hipMemcpyAsync(hcodes.data(), mw.hcodes.p, n * 4, hipMemcpyDeviceToHost, s));
  HG_CHECK(c, sub.finish());
  HG_CHECK(c, hipStreamSynchronize(s));
  // a message that cannot be hashed has no point (the device holds a placeholder)
  for (size_t i = 0; i < n; i++)
    if (hcodes[i] != HG_OK) memset(out + 64 * i, 0, 64);
  return HG_OK;
}

}  // extern "C"
