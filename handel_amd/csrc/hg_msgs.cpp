// hg_msgs.cpp — the C ABI's batches whose checks each carry their own message
// (include/handel_gpu.h: hg_verify_batch_msgs*, hg_hash_messages and the two
// probes) and whose aggregate requests do (hg_verify_aggregate_msgs*,
// hg_verify_multisig_msgs: VerifyMultiSignature(msg, ...), crypto.go:120-137).
// The reference's PublicKey.VerifySignature takes the message per
// call (bn256/go/bn256.go:82-94); here hashedMessage (bn256/go/bn256.go:210-218)
// runs for every check on the device (bn256_msgs.hip) and the pairing kernels
// read H per check. Nothing below touches the context's messages (hg_ctx::cur,
// alt), their H or their GT tables.
#include <cstdio>
#include <vector>

#include "hg_aggregate.h"
#include "hg_sha256.h"

// the G1 base table, built by the context's first multi-message submission
// (inside it: later submissions on other streams wait for this one's event)
int ensure_g1_table(hg_ctx* c, hipStream_t s) {
  if (c->msgs.g1_tab.p) return HG_OK;
  HG_CHECK(c, c->msgs.g1_tab.alloc(kG1TabEntries));
  launch_g1_base_table(c->msgs.g1_tab.p, s);
  int rc = check_launch(c);
  if (rc) c->msgs.g1_tab.reset();
  return rc;
}

// k and hcodes of n pooled messages, then H per check (all in c->msgs)
static int hash_device_locked(hg_ctx* c, const uint8_t* d_pool, size_t pool_len, const uint32_t* d_off,
                              const uint32_t* d_len, size_t n, hipStream_t s) {
  HG_CHECK(c, c->msgs.k.ensure(8 * n));
  HG_CHECK(c, c->msgs.hcodes.ensure(n));
  HG_CHECK(c, c->msgs.h.ensure(n));
  int rc = ensure_g1_table(c, s);
  if (rc) return rc;
  launch_hash_scalars(d_pool, pool_len, d_off, d_len, (int)n, c->msgs.k.p, c->msgs.hcodes.p, s);
  launch_hash_points(c->msgs.k.p, c->msgs.hcodes.p, (int)n, c->msgs.g1_tab.p, c->msgs.h.p, s);
  return check_launch(c);
}

static int verify_msgs_device_locked(hg_ctx* c, const uint8_t* d_pool, size_t pool_len, const uint32_t* d_off,
                                     const uint32_t* d_len, const uint8_t* d_pks, const uint8_t* d_sigs, size_t n,
                                     int32_t* d_codes, hipStream_t s) {
  HG_CHECK(c, c->ws.checks.ensure(n));
  const bool split = verify_split_for(c->verify_split, n);
  if (split) HG_CHECK(c, c->ws.sig_lines.ensure(verify_split_ws_bytes((int)n)));
  Submission sub(c, s);
  HG_CHECK(c, sub.start());
  PhaseTimer all(c, HG_PHASE_SUBMIT, s);
  int rc = hash_device_locked(c, d_pool, pool_len, d_off, d_len, n, s);
  if (rc) return rc;
  // precedence: unmarshal of pk, of sig > hashedMessage's EOF > verdict
  launch_decode_checks(d_pks, d_sigs, (int)n, c->flavor, c->ws.checks.p, d_codes, s);
  launch_merge_hash_codes(c->msgs.hcodes.p, (int)n, d_codes, s);
  PhaseTimer t(c, HG_PHASE_VERIFY, s);
  if (!split) launch_verify_msgs(c->ws.checks.p, (int)n, c->d_lines.p, c->msgs.h.p, d_codes, s);
  else if (!launch_verify_msgs_split(c->ws.checks.p, (int)n, c->d_lines.p, c->msgs.h.p, d_codes, c->ws.sig_lines.p, s)) {
    c->err = "hg_verify_batch_msgs: batch too large for the split form";
    return HG_ERR_ARG;
  }
  t.stop();
  all.stop();
  rc = check_launch(c);
  if (rc) return rc;
  HG_CHECK(c, sub.finish());
  return HG_OK;
}

// the host variants' argument check: every range inside the pool
int check_ranges(hg_ctx* c, const char* who, size_t pool_len, const uint32_t* off, const uint32_t* len, size_t n) {
  if (pool_len >= ((uint64_t)1 << 32)) {
    c->err = std::string(who) + ": pool_len must be below 2^32";
    return HG_ERR_ARG;
  }
  for (size_t i = 0; i < n; i++) {
    if ((uint64_t)off[i] + len[i] <= pool_len) continue;
    char buf[160];
    snprintf(buf, sizeof buf, "%s: message %zu (offset %u, length %u) leaves the pool of %zu bytes", who, i, off[i],
             len[i], pool_len);
    c->err = buf;
    return HG_ERR_ARG;
  }
  return HG_OK;
}

// pool, offsets and lengths to the device (c->stream, inside the caller's submission)
int stage_messages(hg_ctx* c, const uint8_t* pool, size_t pool_len, const uint32_t* off, const uint32_t* len,
                   size_t n) {
  HG_CHECK(c, c->msgs.pool.ensure(pool_len));
  HG_CHECK(c, c->msgs.off.ensure(n));
  HG_CHECK(c, c->msgs.len.ensure(n));
  if (pool_len) HG_CHECK(c, hipMemcpyAsync(c->msgs.pool.p, pool, pool_len, hipMemcpyHostToDevice, c->stream));
  HG_CHECK(c, hipMemcpyAsync(c->msgs.off.p, off, n * 4, hipMemcpyHostToDevice, c->stream));
  HG_CHECK(c, hipMemcpyAsync(c->msgs.len.p, len, n * 4, hipMemcpyHostToDevice, c->stream));
  return HG_OK;
}

// ---------------------------------------------------------------- aggregate requests on their own messages
// hg_verify_aggregate_msgs*: verifySignature (processing.go:342-368) and
// VerifyMultiSignature (crypto.go:120-137) with the message per request. GT
// tables are e(H, pk_i) for one H, so they cannot serve this path: every batch
// runs the level-0 flow of hg_aggregate.cpp (flow_g2_or_mixed), the G2 fold and
// the two-pairing check, with the check reading H per request:
//   s:    level codes, G2 fold into ws.checks ......... -> wait -> merge -> k_msgs_verify (-> keys out)
//   side: wait -> k_hash_scalars, k_hash_points -> join
// The hash depends on nothing the fold produces (one latency-bound chain per
// wave), so it runs on the workspace's side stream beside the fold;
// hg_set_fold_overlap(ctx, 0) runs it first on s (same codes, for measuring).
// The pairing always runs in the one-kernel form here, whatever
// hg_set_verify_split says: the split form's Miller kernel ran 1.20 ms in
// bn256_msgs.hip's unit against 0.75 ms for identical code elsewhere, cause not
// found, so this path does not offer it.
int aggregate_msgs_device_locked(hg_ctx* c, const uint8_t* d_pool, size_t pool_len, const uint32_t* d_off,
                                 const uint32_t* d_len, const hg_request* d_reqs, size_t n, const uint64_t* d_words,
                                 const uint8_t* d_sigs, int32_t* d_codes, uint8_t* d_agg, hipStream_t s) {
  if (c->nreg == 0) {
    c->err = "hg_verify_aggregate_msgs: needs a registry";
    return HG_ERR_ARG;
  }
  Ws& ws = c->ws;
  const bool beside = c->pol.overlap;
  HG_CHECK(c, ws.checks.ensure(n));
  HG_CHECK(c, ws.order.ensure(n));
  HG_CHECK(c, ws.agg_ws.ensure(n * agg_partial_bytes() + agg_fixed_bytes()));
  HG_CHECK(c, ws.codes_c.ensure(n));
  if (d_agg) HG_CHECK(c, ws.pts2.ensure(n));
  if (beside) HG_CHECK(c, ensure_side(ws));
  Submission sub(c, s);
  HG_CHECK(c, sub.start());
  PhaseTimer all(c, HG_PHASE_SUBMIT, s);
  const hipStream_t hs = beside ? ws.side.h : s;
  if (beside) {
    HG_CHECK(c, hipEventRecord(ws.ev_fork, s));
    HG_CHECK(c, hipStreamWaitEvent(hs, ws.ev_fork, 0));
  }
  int rc = hash_device_locked(c, d_pool, pool_len, d_off, d_len, n, hs);
  if (beside) HG_CHECK(c, hipEventRecord(ws.ev_join, hs));
  if (rc) {
    if (beside) (void)hipStreamWaitEvent(s, ws.ev_join, 0);  // the submission's end covers the side stream
    return rc;
  }
  launch_aggmsgs_levels(d_reqs, (int)n, (uint32_t)c->nreg, ws.codes_c.p, s);
  PhaseTimer fold(c, HG_PHASE_AGGREGATE, s);
  launch_aggregate(c->wsum.p, (int)c->nreg, c->blocks.p, c->block_base.data(), c->block_levels, d_reqs, (int)n, d_words,
                   ws.order.p, ws.agg_ws.p, ws.checks.p, ws.codes_c.p, s);
  fold.stop();
  if (beside) HG_CHECK(c, hipStreamWaitEvent(s, ws.ev_join, 0));
  launch_aggmsgs_merge(d_sigs, (int)n, c->flavor, ws.codes_c.p, c->msgs.hcodes.p, ws.checks.p, d_codes, s);
  PhaseTimer t(c, HG_PHASE_VERIFY, s);
  launch_verify_msgs(ws.checks.p, (int)n, c->d_lines.p, c->msgs.h.p, d_codes, s);
  t.stop();
  if (d_agg) {
    launch_extract_pk(ws.checks.p, (int)n, ws.pts2.p, s);
    launch_encode_g2(ws.pts2.p, (int)n, d_agg, s);
  }
  all.stop();
  rc = check_launch(c);
  if (rc) return rc;
  HG_CHECK(c, sub.finish());
  return HG_OK;
}

// the host variants: every argument check before anything is launched, then
// the batch staged on the context's stream (HostStage, hg_aggregate.h) with
// its messages. multisig: the requests are VerifyMultiSignature's
// (multisig_requests), whose size check (crypto.go:121-124) has its own code:
// the level error alone is renamed here.
static int aggregate_msgs_host_locked(hg_ctx* c, const uint8_t* pool, size_t pool_len, const uint32_t* off,
                                      const uint32_t* len, const HostBatch& h, int32_t* codes, uint8_t* agg_out,
                                      bool multisig) {
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
  rc = st.open(h, agg_out != nullptr);
  if (rc == HG_OK) rc = stage_messages(c, pool, pool_len, off, len, n);
  if (rc) return rc;
  const AggBatch b = st.batch(h);
  rc = aggregate_msgs_device_locked(c, c->msgs.pool.p, pool_len, c->msgs.off.p, c->msgs.len.p, b.reqs, n, b.words,
                                    b.sigs, b.codes, b.agg, c->stream);
  if (rc == HG_OK) rc = st.close(h, b.codes, codes, agg_out);
  if (rc) return rc;
  if (multisig)
    for (size_t i = 0; i < n; i++)
      if (codes[i] == HG_ERR_LEVEL) codes[i] = HG_ERR_MULTI_SIZES;
  return HG_OK;
}

extern "C" {

int hg_verify_aggregate_msgs_device(hg_ctx* c, const uint8_t* d_pool, size_t pool_len, const uint32_t* d_msg_off,
                                    const uint32_t* d_msg_len, const hg_request* d_reqs, size_t n,
                                    const uint64_t* d_words, const uint8_t* d_sigs, int32_t* d_codes,
                                    uint8_t* d_agg_pk_out, void* stream) {
  if (!c || (n && (!d_msg_off || !d_msg_len || !d_reqs || !d_sigs || !d_codes)) || (!d_pool && pool_len) ||
      n > (size_t)INT32_MAX)
    return HG_ERR_ARG;
  if (n == 0) return HG_OK;
  std::lock_guard<std::mutex> g(c->mu);
  HG_CHECK(c, hipSetDevice(c->device));
  hipStream_t s = stream ? (hipStream_t)stream : c->stream;
  return aggregate_msgs_device_locked(c, d_pool, pool_len, d_msg_off, d_msg_len, d_reqs, n, d_words, d_sigs, d_codes,
                                      d_agg_pk_out, s);
}

int hg_verify_aggregate_msgs(hg_ctx* c, const uint8_t* pool, size_t pool_len, const uint32_t* msg_off,
                             const uint32_t* msg_len, const hg_request* reqs, size_t n, const uint64_t* words,
                             size_t nwords, const uint8_t* sigs, int32_t* codes, uint8_t* agg_pk_out) {
  if (!c || (n && (!msg_off || !msg_len || !reqs || !sigs || !codes)) || (!pool && pool_len) || (!words && nwords) ||
      n > (size_t)INT32_MAX)
    return HG_ERR_ARG;
  if (n == 0) return HG_OK;
  std::lock_guard<std::mutex> g(c->mu);
  return aggregate_msgs_host_locked(c, pool, pool_len, msg_off, msg_len,
                                    HostBatch{"hg_verify_aggregate_msgs", reqs, n, words, nwords, sigs}, codes,
                                    agg_pk_out, false);
}

int hg_verify_multisig_msgs(hg_ctx* c, const uint8_t* pool, size_t pool_len, const uint32_t* msg_off,
                            const uint32_t* msg_len, const uint32_t* bitlens, const uint32_t* word_offsets, size_t n,
                            const uint64_t* words, size_t nwords, const uint8_t* sigs, int32_t* codes) {
  if (!c || (n && (!msg_off || !msg_len || !bitlens || !word_offsets || !sigs || !codes)) || (!pool && pool_len) ||
      (!words && nwords) || n > (size_t)INT32_MAX)
    return HG_ERR_ARG;
  if (n == 0) return HG_OK;
  std::lock_guard<std::mutex> g(c->mu);
  // crypto.go:121-124: the bitset must span the registry (bitlen != N is the
  // level error of the request [0, N), renamed); the rest is verifySignature
  const std::vector<hg_request> reqs = multisig_requests(c, bitlens, word_offsets, n);
  return aggregate_msgs_host_locked(c, pool, pool_len, msg_off, msg_len,
                                    HostBatch{"hg_verify_multisig_msgs", reqs.data(), n, words, nwords, sigs}, codes,
                                    nullptr, true);
}

int hg_verify_batch_msgs_device(hg_ctx* c, const uint8_t* d_pool, size_t pool_len, const uint32_t* d_msg_off,
                                const uint32_t* d_msg_len, const uint8_t* d_pks, const uint8_t* d_sigs, size_t n,
                                int32_t* d_codes, void* stream) {
  if (!c || (n && (!d_msg_off || !d_msg_len || !d_pks || !d_sigs || !d_codes)) || (!d_pool && pool_len) ||
      n > (size_t)INT32_MAX)
    return HG_ERR_ARG;
  if (n == 0) return HG_OK;
  std::lock_guard<std::mutex> g(c->mu);
  HG_CHECK(c, hipSetDevice(c->device));
  hipStream_t s = stream ? (hipStream_t)stream : c->stream;
  return verify_msgs_device_locked(c, d_pool, pool_len, d_msg_off, d_msg_len, d_pks, d_sigs, n, d_codes, s);
}

int hg_verify_batch_msgs(hg_ctx* c, const uint8_t* pool, size_t pool_len, const uint32_t* msg_off,
                         const uint32_t* msg_len, const uint8_t* pks, const uint8_t* sigs, size_t n, int32_t* codes) {
  if (!c || (n && (!msg_off || !msg_len || !pks || !sigs || !codes)) || (!pool && pool_len) || n > (size_t)INT32_MAX)
    return HG_ERR_ARG;
  if (n == 0) return HG_OK;
  std::lock_guard<std::mutex> g(c->mu);
  int rc = check_ranges(c, "hg_verify_batch_msgs", pool_len, msg_off, msg_len, n);
  if (rc) return rc;
  HG_CHECK(c, hipSetDevice(c->device));
  HG_CHECK(c, c->bytes_a.ensure(n * 128));
  HG_CHECK(c, c->bytes_b.ensure(n * 64));
  HG_CHECK(c, c->ws.codes_c.ensure(n));
  Submission sub(c, c->stream);
  HG_CHECK(c, sub.start());
  rc = stage_messages(c, pool, pool_len, msg_off, msg_len, n);
  if (rc) return rc;
  HG_CHECK(c, hipMemcpyAsync(c->bytes_a.p, pks, n * 128, hipMemcpyHostToDevice, c->stream));
  HG_CHECK(c, hipMemcpyAsync(c->bytes_b.p, sigs, n * 64, hipMemcpyHostToDevice, c->stream));
  rc = verify_msgs_device_locked(c, c->msgs.pool.p, pool_len, c->msgs.off.p, c->msgs.len.p, c->bytes_a.p,
                                 c->bytes_b.p, n, c->ws.codes_c.p, c->stream);
  if (rc) return rc;
  HG_CHECK(c, hipMemcpyAsync(codes, c->ws.codes_c.p, n * 4, hipMemcpyDeviceToHost, c->stream));
  HG_CHECK(c, sub.finish());
  HG_CHECK(c, hipStreamSynchronize(c->stream));
  return HG_OK;
}

int hg_hash_messages(hg_ctx* c, const uint8_t* pool, size_t pool_len, const uint32_t* msg_off,
                     const uint32_t* msg_len, size_t n, uint8_t* h_out, int32_t* codes) {
  if (!c || (n && (!msg_off || !msg_len || !h_out || !codes)) || (!pool && pool_len) || n > (size_t)INT32_MAX)
    return HG_ERR_ARG;
  if (n == 0) return HG_OK;
  std::lock_guard<std::mutex> g(c->mu);
  int rc = check_ranges(c, "hg_hash_messages", pool_len, msg_off, msg_len, n);
  if (rc) return rc;
  HG_CHECK(c, hipSetDevice(c->device));
  HG_CHECK(c, c->bytes_a.ensure(n * 64));
  Submission sub(c, c->stream);
  HG_CHECK(c, sub.start());
  rc = stage_messages(c, pool, pool_len, msg_off, msg_len, n);
  if (rc) return rc;
  rc = hash_device_locked(c, c->msgs.pool.p, pool_len, c->msgs.off.p, c->msgs.len.p, n, c->stream);
  if (rc) return rc;
  launch_encode_g1(c->msgs.h.p, (int)n, c->bytes_a.p, c->stream);
  rc = check_launch(c);
  if (rc) return rc;
  HG_CHECK(c, hipMemcpyAsync(h_out, c->bytes_a.p, n * 64, hipMemcpyDeviceToHost, c->stream));
  HG_CHECK(c, hipMemcpyAsync(codes, c->msgs.hcodes.p, n * 4, hipMemcpyDeviceToHost, c->stream));
  HG_CHECK(c, sub.finish());
  HG_CHECK(c, hipStreamSynchronize(c->stream));
  return HG_OK;
}

int hg_debug_g1_base_mul(hg_ctx* c, const uint32_t* k_words, size_t n, uint8_t* out) {
  if (!c || (n && (!k_words || !out)) || n > (size_t)INT32_MAX) return HG_ERR_ARG;
  if (n == 0) return HG_OK;
  std::lock_guard<std::mutex> g(c->mu);
  HG_CHECK(c, hipSetDevice(c->device));
  HG_CHECK(c, c->bytes_a.ensure(n * 64));
  HG_CHECK(c, c->msgs.k.ensure(8 * n));
  HG_CHECK(c, c->msgs.h.ensure(n));
  Submission sub(c, c->stream);
  HG_CHECK(c, sub.start());
  int rc = ensure_g1_table(c, c->stream);
  if (rc) return rc;
  HG_CHECK(c, hipMemcpyAsync(c->msgs.k.p, k_words, n * 32, hipMemcpyHostToDevice, c->stream));
  launch_hash_points(c->msgs.k.p, nullptr, (int)n, c->msgs.g1_tab.p, c->msgs.h.p, c->stream);
  launch_encode_g1(c->msgs.h.p, (int)n, c->bytes_a.p, c->stream);
  rc = check_launch(c);
  if (rc) return rc;
  HG_CHECK(c, hipMemcpyAsync(out, c->bytes_a.p, n * 64, hipMemcpyDeviceToHost, c->stream));
  HG_CHECK(c, sub.finish());
  HG_CHECK(c, hipStreamSynchronize(c->stream));
  return HG_OK;
}

int hg_debug_hash_scalar(const uint8_t* msg, size_t len, uint32_t k[8]) {
  if ((!msg && len) || !k) return HG_ERR_ARG;
  uint32_t h[8];
  sha256_words(msg, len, h);
  return hash_scalar_words(h, k) ? HG_OK : HG_ERR_HASH_EOF;
}

}  // extern "C"
