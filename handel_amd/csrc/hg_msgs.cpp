// hg_msgs.cpp — the C ABI's batches whose checks each carry their own message
// (include/handel_gpu.h: hg_verify_batch_msgs*, hg_hash_messages and the two
// probes). The reference's PublicKey.VerifySignature takes the message per
// call (bn256/go/bn256.go:82-94); here hashedMessage (bn256/go/bn256.go:210-218)
// runs for every check on the device (bn256_msgs.hip) and the pairing kernels
// read H per check. Nothing below touches the context's messages (hg_ctx::cur,
// alt), their H or their GT tables.
#include <cstdio>

#include "hg_ctx.h"
#include "hg_sha256.h"

// the G1 base table, built by the context's first multi-message submission
// (inside it: later submissions on other streams wait for this one's event)
static int ensure_g1_table(hg_ctx* c, hipStream_t s) {
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
static int check_ranges(hg_ctx* c, const char* who, size_t pool_len, const uint32_t* off, const uint32_t* len,
                        size_t n) {
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
static int stage_messages(hg_ctx* c, const uint8_t* pool, size_t pool_len, const uint32_t* off, const uint32_t* len,
                          size_t n) {
  HG_CHECK(c, c->msgs.pool.ensure(pool_len));
  HG_CHECK(c, c->msgs.off.ensure(n));
  HG_CHECK(c, c->msgs.len.ensure(n));
  if (pool_len) HG_CHECK(c, hipMemcpyAsync(c->msgs.pool.p, pool, pool_len, hipMemcpyHostToDevice, c->stream));
  HG_CHECK(c, hipMemcpyAsync(c->msgs.off.p, off, n * 4, hipMemcpyHostToDevice, c->stream));
  HG_CHECK(c, hipMemcpyAsync(c->msgs.len.p, len, n * 4, hipMemcpyHostToDevice, c->stream));
  return HG_OK;
}

extern "C" {

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
