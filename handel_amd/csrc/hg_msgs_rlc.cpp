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

#include "bn256_brlc.h"
#include "bn256_sigform.h"
#include "hg_aggregate.h"

// ---------------------------------------------------------------- the combined flow (MrlcFlow, hg_aggregate.h)
// of checks that carry a message each: this file's requests and hg_batch_rlc.cpp's independent checks
namespace {

hipError_t mrlc_ensure(hg_ctx* c, size_t n, size_t ng, bool members) {
  Ws& ws = c->ws;
  MsgWs& mw = c->msgs;
  hipError_t e = hipSuccess;
  auto grow = [&e](auto& buf, size_t count) {
    if (e == hipSuccess) e = buf.ensure(count);
  };
  // the exact flows'
  grow(ws.checks, n), grow(mw.k, 8 * n), grow(mw.hcodes, n), grow(mw.h, n);
  // the combination's
  grow(ws.pts1, n), grow(ws.rlc_r, n), grow(ws.rlc_jac, n);
  grow(ws.rlc_glive, ng), grow(ws.rlc_gcodes, ng), grow(ws.rlc_gpts, ng), grow(ws.rlc_z, ng), grow(ws.rlc_hdr, 1);
  grow(ws.sig_lines, fe12_ws_bytes((int)ng));
  grow(mw.rk, 8 * n), grow(mw.rh, n), grow(mw.rchecks, n), grow(mw.f, n), grow(mw.carrier, ng);
  if (members) grow(mw.member, n);
  return e;
}

// The failed groups' live members through the exact check: gathered in index
// order with their unscaled H, verified as a batch of their own, the codes
// scattered back.
int mrlc_recheck(hg_ctx* c, int32_t* codes, size_t n, uint32_t group, size_t m, hipStream_t s) {
  Ws& ws = c->ws;
  MsgWs& mw = c->msgs;
  HG_CHECK(c, ws.rlc_bcount.ensure((n + 255) / 256));
  HG_CHECK(c, ws.rlc_idx.ensure(m));
  HG_CHECK(c, ws.rlc_ccodes.ensure(m));
  HG_CHECK(c, mw.cchecks.ensure(m));
  HG_CHECK(c, mw.ch.ensure(m));
  launch_mrlc_gather(codes, ws.rlc_gcodes.p, (int)n, group, ws.checks.p, mw.h.p, ws.rlc_bcount.p, ws.rlc_idx.p,
                     mw.cchecks.p, mw.ch.p, ws.rlc_ccodes.p, s);
  launch_verify_msgs(mw.cchecks.p, (int)m, c->d_lines.p, mw.ch.p, ws.rlc_ccodes.p, s);
  launch_rlc_scatter(ws.rlc_idx.p, ws.rlc_ccodes.p, (int)m, codes, s);
  return HG_OK;
}

// The hash stream's end: its join record; after an error the wait for it as
// well, so that the submission's end covers the side stream.
int mrlc_join(MrlcFlow& f, int rc) {
  hg_ctx* c = f.c;
  if (f.hs == f.s) return rc;
  HG_CHECK(c, hipEventRecord(c->ws.ev_join, f.hs));
  if (rc) (void)hipStreamWaitEvent(f.s, c->ws.ev_join, 0);
  return rc;
}

}  // namespace

int mrlc_begin(MrlcFlow& f) {
  hg_ctx* c = f.c;
  Ws& ws = c->ws;
  const bool beside = c->pol.overlap;
  HG_CHECK(c, mrlc_ensure(c, f.n, f.ng(), f.members));
  if (beside) HG_CHECK(c, ensure_side(ws));
  HG_CHECK(c, f.sub.start());
  f.all.emplace(c, HG_PHASE_SUBMIT, f.s);
  launch_rlc_prep(rlc_seed_of(f.call.seed), f.call.d_coeffs, (int)f.n, (int)f.ng(), ws.rlc_r.p, ws.rlc_gcodes.p,
                  ws.rlc_hdr.p, f.s);
  f.hs = beside ? ws.side.h : f.s;
  if (beside) {
    HG_CHECK(c, hipEventRecord(ws.ev_fork, f.s));
    HG_CHECK(c, hipStreamWaitEvent(f.hs, ws.ev_fork, 0));
  }
  const int rc = ensure_g1_table(c, f.hs);
  return rc ? mrlc_join(f, rc) : HG_OK;
}

int mrlc_hashed(MrlcFlow& f) {
  hg_ctx* c = f.c;
  MsgWs& mw = c->msgs;
  // H_i (the caller's) for the recheck and r_i H_i for the combination: two walks
  // of the fixed-base table, no G1 chain and no inversion more than that
  launch_mrlc_scalars(mw.k.p, mw.hcodes.p, c->ws.rlc_r.p, (int)f.n, mw.rk.p, f.hs);
  launch_hash_points(mw.rk.p, mw.hcodes.p, (int)f.n, mw.g1_tab.p, mw.rh.p, f.hs);
  return mrlc_join(f, check_launch(c));
}

int mrlc_wait_hashed(MrlcFlow& f) {
  if (f.hs != f.s) HG_CHECK(f.c, hipStreamWaitEvent(f.s, f.c->ws.ev_join, 0));
  return HG_OK;
}

int mrlc_finish(MrlcFlow& f, int32_t* codes) {
  hg_ctx* c = f.c;
  Ws& ws = c->ws;
  MsgWs& mw = c->msgs;
  const hipStream_t s = f.s;
  const int n = (int)f.n, ng = (int)f.ng();
  const uint32_t group = f.call.group;
  PhaseTimer t(c, HG_PHASE_VERIFY, s);
  // sum r_i sig_i per group over the live members
  launch_mrlc_sigs(ws.checks.p, n, ws.pts1.p, s);
  launch_rlc_g1_mul(ws.pts1.p, codes, ws.rlc_r.p, n, ws.rlc_jac.p, s);
  launch_rlc_g1_sum(ws.rlc_jac.p, codes, n, group, ng, ws.rlc_gpts.p, ws.rlc_glive.p, s);
  launch_mrlc_checks(ws.checks.p, codes, ws.rlc_gpts.p, n, group, ng, mw.carrier.p, mw.rchecks.p, s);
  if (f.members) launch_brlc_miller(mw.rchecks.p, n, c->d_lines.p, mw.rh.p, 1, mw.f.p, mw.member.p, s);
  else launch_mrlc_miller(mw.rchecks.p, n, c->d_lines.p, mw.rh.p, mw.f.p, s);
  launch_mrlc_product(mw.f.p, codes, n, group, ng, ws.rlc_z.p, s);
  if (!launch_fe12(ws.rlc_z.p, ng, ws.sig_lines.p, s)) {
    c->err = std::string(f.call.who) + ": too many groups for the final exponentiation";
    return HG_ERR_ARG;
  }
  launch_fe_verdicts(ws.rlc_z.p, ng, ws.rlc_gcodes.p, s);
  // a group is accepted only if every live key of it is proven in G2
  if (f.members) launch_brlc_members(codes, mw.member.p, n, group, ng, ws.rlc_gcodes.p, ws.rlc_hdr.p, s);
  launch_rlc_count(ws.rlc_gcodes.p, ws.rlc_glive.p, ng, ws.rlc_hdr.p, s);
  int rc = check_launch(c);
  if (rc) return rc;
  if (f.call.recheck) {
    rc = rlc_read_stats(c, f.call, f.n, s, &f.hdr);
    if (rc == HG_OK && f.hdr.failed_members) rc = mrlc_recheck(c, codes, f.n, group, f.hdr.failed_members, s);
    if (rc) return rc;
  }
  t.stop();
  f.all->stop();
  rc = check_launch(c);
  if (rc) return rc;
  HG_CHECK(c, f.sub.finish());
  return HG_OK;
}

// ---------------------------------------------------------------- hg_verify_aggregate_msgs_rlc* and the probes
namespace {

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

// One batch on stream s with the context's workspaces (the streams: MrlcFlow,
// hg_aggregate.h). *ran: the combination ran (false: the exact call did).
int mrlc_device_locked(hg_ctx* c, const MsgBatch& b, const RlcCall& call, bool* ran, hipStream_t s) {
  *ran = false;
  rlc_clear_stats(c);
  if (c->nreg == 0) {
    c->err = std::string(call.who) + ": needs a registry";
    return HG_ERR_ARG;
  }
  const size_t n = b.n;
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
  // the exact flow's fold
  HG_CHECK(c, ws.order.ensure(n));
  HG_CHECK(c, ws.agg_ws.ensure(n * agg_partial_bytes() + agg_fixed_bytes()));
  HG_CHECK(c, ws.codes_c.ensure(n));
  MrlcFlow f(c, call, n, false, s);
  rc = mrlc_begin(f);
  if (rc) return rc;
  // H_i: every request's own message hashed
  launch_hash_scalars(b.pool, b.pool_len, b.off, b.len, (int)n, mw.k.p, mw.hcodes.p, f.hs);
  launch_hash_points(mw.k.p, mw.hcodes.p, (int)n, mw.g1_tab.p, mw.h.p, f.hs);
  rc = mrlc_hashed(f);
  if (rc) return rc;
  launch_aggmsgs_levels(b.reqs, (int)n, (uint32_t)c->nreg, ws.codes_c.p, s);
  PhaseTimer fold(c, HG_PHASE_AGGREGATE, s);
  launch_aggregate(c->wsum.p, (int)c->nreg, c->blocks.p, c->block_base.data(), c->block_levels, b.reqs, (int)n, b.words,
                   ws.order.p, ws.agg_ws.p, ws.checks.p, ws.codes_c.p, s);
  fold.stop();
  rc = mrlc_wait_hashed(f);
  if (rc) return rc;
  launch_aggmsgs_merge(b.sigs, (int)n, c->flavor, ws.codes_c.p, mw.hcodes.p, ws.checks.p, b.codes, s);
  rc = mrlc_finish(f, b.codes);
  *ran = rc == HG_OK;
  return rc;
}

// host pointers in, through the context's staging buffers (as hg_verify_aggregate_msgs)
int mrlc_host_locked(hg_ctx* c, const uint8_t* pool, size_t pool_len, const uint32_t* off, const uint32_t* len,
                     const HostBatch& h, const uint64_t* coeffs, const RlcCall& call0, int32_t* codes,
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
  RlcCall call = call0;
  call.d_coeffs = coeffs ? reinterpret_cast<const uint64_t*>(c->bytes_a.p) : nullptr;
  const AggBatch ab = st.batch(h);
  const MsgBatch b{c->msgs.pool.p, pool_len, c->msgs.off.p, c->msgs.len.p, ab.reqs, n, ab.words, ab.sigs, ab.codes};
  bool ran = false;
  rc = mrlc_device_locked(c, b, call, &ran, c->stream);
  if (rc) return rc;
  if (group_codes && ran) {
    rc = rlc_copy_groups(c, rlc_groups(n, call.group), group_codes, group_live, c->stream);
    if (rc) return rc;
  }
  return st.close(h, b.codes, codes, nullptr);
}

}  // namespace

extern "C" {

int hg_verify_aggregate_msgs_rlc(hg_ctx* c, const uint8_t* pool, size_t pool_len, const uint32_t* msg_off,
                                 const uint32_t* msg_len, const hg_request* reqs, size_t n, const uint64_t* words,
                                 size_t nwords, const uint8_t* sigs, const uint8_t seed[32], uint32_t group,
                                 int32_t* codes) {
  if (!c || !seed || !rlc_group_ok(group) || (n && (!msg_off || !msg_len || !reqs || !sigs || !codes)) ||
      (!pool && pool_len) || (!words && nwords) || n > (size_t)INT32_MAX)
    return HG_ERR_ARG;
  std::lock_guard<std::mutex> g(c->mu);
  rlc_clear_stats(c);
  if (n == 0) return HG_OK;
  return mrlc_host_locked(c, pool, pool_len, msg_off, msg_len,
                          HostBatch{"hg_verify_aggregate_msgs_rlc", reqs, n, words, nwords, sigs}, nullptr,
                          RlcCall{"hg_verify_aggregate_msgs_rlc", seed, nullptr, group, true}, codes, nullptr, nullptr);
}

int hg_verify_aggregate_msgs_rlc_device(hg_ctx* c, const uint8_t* d_pool, size_t pool_len, const uint32_t* d_msg_off,
                                        const uint32_t* d_msg_len, const hg_request* d_reqs, size_t n,
                                        const uint64_t* d_words, const uint8_t* d_sigs, const uint8_t seed[32],
                                        uint32_t group, int32_t* d_codes, void* stream) {
  if (!c || !seed || !rlc_group_ok(group) || (n && (!d_msg_off || !d_msg_len || !d_reqs || !d_sigs || !d_codes)) ||
      (!d_pool && pool_len) || n > (size_t)INT32_MAX)
    return HG_ERR_ARG;
  std::lock_guard<std::mutex> g(c->mu);
  rlc_clear_stats(c);
  if (n == 0) return HG_OK;
  HG_CHECK(c, hipSetDevice(c->device));
  hipStream_t s = stream ? (hipStream_t)stream : c->stream;
  bool ran = false;
  return mrlc_device_locked(c, MsgBatch{d_pool, pool_len, d_msg_off, d_msg_len, d_reqs, n, d_words, d_sigs, d_codes},
                            RlcCall{"hg_verify_aggregate_msgs_rlc_device", seed, nullptr, group, true}, &ran, s);
}

int hg_verify_multisig_msgs_rlc(hg_ctx* c, const uint8_t* pool, size_t pool_len, const uint32_t* msg_off,
                                const uint32_t* msg_len, const uint32_t* bitlens, const uint32_t* word_offsets,
                                size_t n, const uint64_t* words, size_t nwords, const uint8_t* sigs,
                                const uint8_t seed[32], uint32_t group, int32_t* codes) {
  if (!c || !seed || !rlc_group_ok(group) ||
      (n && (!msg_off || !msg_len || !bitlens || !word_offsets || !sigs || !codes)) || (!pool && pool_len) ||
      (!words && nwords) || n > (size_t)INT32_MAX)
    return HG_ERR_ARG;
  std::lock_guard<std::mutex> g(c->mu);
  rlc_clear_stats(c);
  if (n == 0) return HG_OK;
  // crypto.go:121-124: the bitset must span the registry (bitlen != N is the
  // level error of the request [0, N), renamed on the host); the rest is verifySignature
  const std::vector<hg_request> reqs = multisig_requests(c, bitlens, word_offsets, n);
  int rc = mrlc_host_locked(c, pool, pool_len, msg_off, msg_len,
                            HostBatch{"hg_verify_multisig_msgs_rlc", reqs.data(), n, words, nwords, sigs}, nullptr,
                            RlcCall{"hg_verify_multisig_msgs_rlc", seed, nullptr, group, true}, codes, nullptr,
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
  if (!c || !rlc_group_ok(group) ||
      (n && (!msg_off || !msg_len || !reqs || !sigs || !coeffs || !codes || !group_codes || !group_live)) ||
      (!pool && pool_len) || (!words && nwords) || n > (size_t)INT32_MAX)
    return HG_ERR_ARG;
  if (n == 0) return HG_OK;
  std::lock_guard<std::mutex> g(c->mu);
  return mrlc_host_locked(c, pool, pool_len, msg_off, msg_len,
                          HostBatch{"hg_debug_msgs_rlc_groups", reqs, n, words, nwords, sigs}, coeffs,
                          RlcCall{"hg_debug_msgs_rlc_groups", nullptr, nullptr, group, false}, codes, group_codes,
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
