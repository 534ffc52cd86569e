// hg_rlc.cpp — hg_verify_aggregate_rlc*: an aggregate batch whose groups of
// checks share one pairing under random coefficients (bn256_rlc.hip, DESIGN.md
// §3l), behind include/handel_gpu.h. The batch runs the prologue and the GT
// fold of the exact path (hg_aggregate.h), then per group the G1 combination,
// the shared-squaring multi-exponentiation of the fold values, one pairing and
// the comparison; the live members of a group that fails go through the exact
// path's stored pairing and comparison. A context that would not take a GT flow
// runs the exact path's table-less flow instead.
#include "hg_aggregate.h"

// ---------------------------------------------------------------- what the three combined forms share (hg_aggregate.h)
void rlc_clear_stats(hg_ctx* c) { c->rlc_stats[0] = c->rlc_stats[1] = c->rlc_stats[2] = 0; }

int rlc_read_stats(hg_ctx* c, const RlcCall& call, size_t n, hipStream_t s, RlcHdr* h) {
  // the one read-back: how many checks the failed groups hold sizes their launch
  RlcHdr got{};
  HG_CHECK(c, hipMemcpyAsync(&got, c->ws.rlc_hdr.p, sizeof got, hipMemcpyDeviceToHost, s));
  HG_CHECK(c, hipStreamSynchronize(s));
  *h = got;
  c->rlc_stats[0] = got.groups;
  c->rlc_stats[1] = got.groups_failed;
  c->rlc_stats[2] = got.failed_members;
  if (got.failed_members > n) {
    c->err = std::string(call.who) + ": inconsistent failed-member count";
    return HG_ERR_DEVICE;
  }
  return HG_OK;
}

int rlc_copy_groups(hg_ctx* c, size_t ng, int32_t* group_codes, uint32_t* group_live, hipStream_t s) {
  HG_CHECK(c, hipMemcpyAsync(group_codes, c->ws.rlc_gcodes.p, ng * 4, hipMemcpyDeviceToHost, s));
  HG_CHECK(c, hipMemcpyAsync(group_live, c->ws.rlc_glive.p, ng * 4, hipMemcpyDeviceToHost, s));
  return HG_OK;
}

// ---------------------------------------------------------------- hg_verify_aggregate_rlc* and the probes
namespace {

hipError_t rlc_ensure(Ws& ws, size_t n, size_t ng) {
  hipError_t e = hipSuccess;
  auto grow = [&e](auto& buf, size_t count) {
    if (e == hipSuccess) e = buf.ensure(count);
  };
  grow(ws.rlc_r, n), grow(ws.rlc_jac, n);
  grow(ws.rlc_glive, ng), grow(ws.rlc_gcodes, ng), grow(ws.rlc_gpts, ng), grow(ws.rlc_gsigs, ng * 64);
  grow(ws.rlc_p, ng * kRlcBits), grow(ws.rlc_z, ng), grow(ws.rlc_hdr, 1);
  return e;
}

// the G1 side's second half: per group the marshal of sum r_i sig_i over the checks whose code is HG_OK
void rlc_g1_sum(Ws& ws, const int32_t* codes, size_t n, uint32_t group, size_t ng, hipStream_t s) {
  launch_rlc_g1_sum(ws.rlc_jac.p, codes, (int)n, group, (int)ng, ws.rlc_gpts.p, ws.rlc_glive.p, s);
  launch_encode_g1(ws.rlc_gpts.p, (int)ng, ws.rlc_gsigs.p, s);
}

// The failed groups' live members through the exact check: gathered in index
// order, paired and compared as a batch of their own, the codes scattered back.
int rlc_recheck(hg_ctx* c, const AggBatch& b, Ws& ws, const GtWork& gw, uint32_t group, size_t m, hipStream_t s) {
  const size_t n = b.n;
  const SigForm form = sig_form(sig_env(), c->pol, m);
  HG_CHECK(c, ws.rlc_bcount.ensure((n + 255) / 256));
  HG_CHECK(c, ws.rlc_idx.ensure(m));
  HG_CHECK(c, ws.rlc_csigs.ensure(m * 64));
  HG_CHECK(c, ws.rlc_cy.ensure(m));
  HG_CHECK(c, ws.rlc_ccodes.ensure(m));
  HG_CHECK(c, ws.sig_lines.ensure(sig_form_ws_bytes(form, (int)m)));
  launch_rlc_gather(b.codes, ws.rlc_gcodes.p, (int)n, group, b.sigs, ws.gt_y.p, ws.rlc_bcount.p, ws.rlc_idx.p,
                    ws.rlc_csigs.p, ws.rlc_cy.p, ws.rlc_ccodes.p, s);
  const AggBatch cb{nullptr, m, nullptr, ws.rlc_csigs.p, ws.rlc_ccodes.p};
  int rc = pair_stored(c, cb, ws, form, s);
  if (rc) return rc;
  if (gw.torus) launch_tor_compare(ws.gt_fe.p, ws.rlc_cy.p, (int)m, ws.rlc_ccodes.p, nullptr, s);
  else launch_gt_compare(ws.gt_fe.p, ws.rlc_cy.p, (int)m, ws.rlc_ccodes.p, s);
  launch_rlc_scatter(ws.rlc_idx.p, ws.rlc_ccodes.p, (int)m, b.codes, s);
  return HG_OK;
}

// One batch on stream s with the context's workspaces. *ran: the combination
// ran (false: the exact path did, or nothing for a probe).
int rlc_device_locked(hg_ctx* c, const AggBatch& b, const RlcCall& call, bool* ran, hipStream_t s) {
  *ran = false;
  rlc_clear_stats(c);
  if (!c->cur.has_msg) {
    c->err = "hg_set_message was not called";
    return HG_ERR_ARG;
  }
  const size_t n = b.n, ng = rlc_groups(n, call.group);
  Ws& ws = c->ws;
  Submission sub(c, s);
  HG_CHECK(c, sub.start());
  int level = 0;
  GtWork gw{};
  int rc = submission_level(c, b, ws, s, true, level, gw);
  if (rc) return rc;
  const SigForm form = sig_form(sig_env(), c->pol, n);
  if (level == 0) {
    // no GT flow: the exact path's fold in G2 and two-pairing check
    if (!call.recheck) {
      c->err = std::string(call.who) + ": the context has no GT tables to combine over";
      return HG_ERR_ARG;
    }
    HG_CHECK(c, ws_ensure(ws, n, kWsG2Fold | kWsVerify | (b.lvl ? 0 : kWsLevel), {}, sig_form_ws_bytes(form, (int)n)));
    PhaseTimer all(c, HG_PHASE_SUBMIT, s);
    rc = flow_g2_or_mixed(c, b, ws, true, false, true, form, gw, s);
    if (rc) return rc;
    all.stop();
    rc = check_launch(c);
    if (rc) return rc;
    HG_CHECK(c, sub.finish());
    return HG_OK;
  }
  const SigForm gform = sig_form(sig_env(), c->pol, ng);
  // The G1 multiples need the decoded signatures and the coefficients only, so
  // they run on the side stream beside the fold and the GT stages (a thread's
  // double-and-add chain is latency no other work of the batch waits for);
  // hg_set_fold_overlap(ctx, 0) keeps everything on one stream.
  const bool beside = c->pol.overlap;
  HG_CHECK(c, ws_ensure(ws, n, kWsVerify | kWsPairing | (beside ? kWsSide : 0), {}, sig_form_ws_bytes(gform, (int)ng)));
  HG_CHECK(c, rlc_ensure(ws, n, ng));
  PhaseTimer all(c, HG_PHASE_SUBMIT, s);
  launch_rlc_prep(rlc_seed_of(call.seed), call.d_coeffs, (int)n, (int)ng, ws.rlc_r.p, ws.rlc_gcodes.p, ws.rlc_hdr.p, s);
  gt_prologue(c, b, ws, gw, s);
  hipStream_t g1s = beside ? (hipStream_t)ws.side : s;
  if (beside) {
    HG_CHECK(c, hipEventRecord(ws.ev_fork, s));
    HG_CHECK(c, hipStreamWaitEvent(ws.side, ws.ev_fork, 0));
  }
  launch_rlc_g1_mul(ws.pts1.p, b.codes, ws.rlc_r.p, (int)n, ws.rlc_jac.p, g1s);
  if (beside) HG_CHECK(c, hipEventRecord(ws.ev_join, ws.side));
  PhaseTimer fold(c, HG_PHASE_AGGREGATE, s);
  gt_fold(c, b, ws, gw, b.codes, false, s);
  fold.stop();
  // the combination's GT stages, a second interval of the phase
  PhaseTimer comb(c, HG_PHASE_AGGREGATE, s);
  launch_rlc_gt(ws.gt_y.p, b.codes, ws.rlc_r.p, (int)n, call.group, (int)ng, ws.rlc_p.p, ws.rlc_z.p, s);
  comb.stop();
  if (beside) HG_CHECK(c, hipStreamWaitEvent(s, ws.ev_join, 0));
  rlc_g1_sum(ws, b.codes, n, call.group, ng, s);
  const AggBatch gb{nullptr, ng, nullptr, ws.rlc_gsigs.p, ws.rlc_gcodes.p};
  rc = pair_stored(c, gb, ws, gform, s);
  if (rc) return rc;
  if (gw.torus) launch_tor_compare(ws.gt_fe.p, ws.rlc_z.p, (int)ng, ws.rlc_gcodes.p, nullptr, s);
  else launch_gt_compare(ws.gt_fe.p, ws.rlc_z.p, (int)ng, ws.rlc_gcodes.p, s);
  launch_rlc_count(ws.rlc_gcodes.p, ws.rlc_glive.p, (int)ng, ws.rlc_hdr.p, s);
  rc = check_launch(c);
  if (rc) return rc;
  *ran = true;
  if (call.recheck) {
    RlcHdr h{};
    rc = rlc_read_stats(c, call, n, s, &h);
    if (rc == HG_OK && h.failed_members) rc = rlc_recheck(c, b, ws, gw, call.group, h.failed_members, s);
    if (rc) return rc;
  }
  all.stop();
  rc = check_launch(c);
  if (rc) return rc;
  HG_CHECK(c, sub.finish());
  return HG_OK;
}

// host pointers in, through the context's staging buffers (as hg_verify_aggregate)
int rlc_host_locked(hg_ctx* c, const HostBatch& h, const uint64_t* coeffs, const RlcCall& call0, int32_t* codes,
                    int32_t* group_codes, uint32_t* group_live) {
  FoldCaps caps;  // exact bounds: the host knows every request's size
  int rc = check_host_requests(c, h, nullptr, &caps);
  if (rc) return rc;
  HostStage st(c);
  rc = st.open(h, false);
  if (rc == HG_OK && coeffs) rc = st.put(c->bytes_a, coeffs, h.n * 8);
  if (rc) return rc;
  RlcCall call = call0;
  call.d_coeffs = coeffs ? reinterpret_cast<const uint64_t*>(c->bytes_a.p) : nullptr;
  AggBatch b = st.batch(h);
  b.caps = &caps;
  bool ran = false;
  rc = rlc_device_locked(c, b, call, &ran, c->stream);
  if (rc) return rc;
  if (group_codes && ran) {
    rc = rlc_copy_groups(c, rlc_groups(h.n, call.group), group_codes, group_live, c->stream);
    if (rc) return rc;
  }
  return st.close(h, b.codes, codes, nullptr);
}

}  // namespace

extern "C" {

int hg_verify_aggregate_rlc(hg_ctx* c, const hg_request* reqs, size_t n, const uint64_t* words, size_t nwords,
                            const uint8_t* sigs, const uint8_t seed[32], uint32_t group, int32_t* codes) {
  if (!c || !seed || !rlc_group_ok(group) || (n && (!reqs || !sigs || !codes)) || n > (size_t)INT32_MAX)
    return HG_ERR_ARG;
  std::lock_guard<std::mutex> g(c->mu);
  rlc_clear_stats(c);
  if (n == 0) return HG_OK;
  return rlc_host_locked(c, HostBatch{"hg_verify_aggregate_rlc", reqs, n, words, nwords, sigs}, nullptr,
                         RlcCall{"hg_verify_aggregate_rlc", seed, nullptr, group, true}, codes, nullptr, nullptr);
}

int hg_verify_aggregate_rlc_device(hg_ctx* c, const hg_request* d_reqs, size_t n, const uint64_t* d_words,
                                   const uint8_t* d_sigs, const uint8_t seed[32], uint32_t group, int32_t* d_codes,
                                   void* stream) {
  if (!c || !seed || !rlc_group_ok(group) || (n && (!d_reqs || !d_sigs || !d_codes)) || n > (size_t)INT32_MAX)
    return HG_ERR_ARG;
  std::lock_guard<std::mutex> g(c->mu);
  rlc_clear_stats(c);
  if (n == 0) return HG_OK;
  HG_CHECK(c, hipSetDevice(c->device));
  hipStream_t s = stream ? (hipStream_t)stream : c->stream;
  bool ran = false;
  // who: hg_last_error names the host variant for both, as it always has
  return rlc_device_locked(c, AggBatch{d_reqs, n, d_words, d_sigs, d_codes},
                           RlcCall{"hg_verify_aggregate_rlc", seed, nullptr, group, true}, &ran, s);
}

int hg_rlc_stats(hg_ctx* c, uint64_t* groups, uint64_t* groups_failed, uint64_t* rechecked) {
  if (!c) return HG_ERR_ARG;
  std::lock_guard<std::mutex> g(c->mu);
  if (groups) *groups = c->rlc_stats[0];
  if (groups_failed) *groups_failed = c->rlc_stats[1];
  if (rechecked) *rechecked = c->rlc_stats[2];
  return HG_OK;
}

int hg_debug_rlc_coeffs(const uint8_t seed[32], uint64_t first, size_t n, uint64_t* out) {
  if (!seed || (n && !out)) return HG_ERR_ARG;
  for (size_t i = 0; i < n; i++) out[i] = rlc_coeff(seed, first + i);
  return HG_OK;
}

int hg_debug_rlc_g1(hg_ctx* c, const uint8_t* sigs, size_t n, const uint64_t* coeffs, uint32_t group,
                    uint8_t* out64_per_group) {
  if (!c || !rlc_group_ok(group) || (n && (!sigs || !coeffs || !out64_per_group)) || n > (size_t)INT32_MAX)
    return HG_ERR_ARG;
  if (n == 0) return HG_OK;
  std::lock_guard<std::mutex> g(c->mu);
  HG_CHECK(c, hipSetDevice(c->device));
  const size_t ng = rlc_groups(n, group);
  Ws& ws = c->ws;
  hipStream_t s = c->stream;
  HG_CHECK(c, c->bytes_b.ensure(n * 64));
  HG_CHECK(c, ws_ensure(ws, n, kWsVerify));
  HG_CHECK(c, rlc_ensure(ws, n, ng));
  Submission sub(c, s);
  HG_CHECK(c, sub.start());
  HG_CHECK(c, hipMemcpyAsync(c->bytes_b.p, sigs, n * 64, hipMemcpyHostToDevice, s));
  HG_CHECK(c, hipMemcpyAsync(ws.rlc_r.p, coeffs, n * 8, hipMemcpyHostToDevice, s));
  launch_decode_g1(c->bytes_b.p, (int)n, c->flavor, ws.pts1.p, ws.codes_b.p, s);
  launch_rlc_g1_mul(ws.pts1.p, ws.codes_b.p, ws.rlc_r.p, (int)n, ws.rlc_jac.p, s);
  rlc_g1_sum(ws, ws.codes_b.p, n, group, ng, s);
  int rc = check_launch(c);
  if (rc) return rc;
  HG_CHECK(c, hipMemcpyAsync(out64_per_group, ws.rlc_gsigs.p, ng * 64, hipMemcpyDeviceToHost, s));
  HG_CHECK(c, sub.finish());
  HG_CHECK(c, hipStreamSynchronize(s));
  return HG_OK;
}

int hg_debug_rlc_groups(hg_ctx* c, const hg_request* reqs, size_t n, const uint64_t* words, size_t nwords,
                        const uint8_t* sigs, const uint64_t* coeffs, uint32_t group, int32_t* codes,
                        int32_t* group_codes, uint32_t* group_live) {
  if (!c || !rlc_group_ok(group) || (n && (!reqs || !sigs || !coeffs || !codes || !group_codes || !group_live)) ||
      n > (size_t)INT32_MAX)
    return HG_ERR_ARG;
  if (n == 0) return HG_OK;
  std::lock_guard<std::mutex> g(c->mu);
  return rlc_host_locked(c, HostBatch{"hg_debug_rlc_groups", reqs, n, words, nwords, sigs}, coeffs,
                         RlcCall{"hg_debug_rlc_groups", nullptr, nullptr, group, false}, codes, group_codes,
                         group_live);
}

}  // extern "C"
