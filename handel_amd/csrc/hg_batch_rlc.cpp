// hg_batch_rlc.cpp — hg_verify_batch_rlc*, hg_verify_batch_msgs_rlc*,
// hg_batch_rlc_stats and their two probes behind include/handel_gpu.h:
// independent PublicKey.VerifySignature checks on arbitrary keys
// (bn256/go/bn256.go:82-94; simul/p2p/aggregator.go:244), on the context's
// message or on a message each, with one final exponentiation per group of
// checks (bn256_batchrlc.hip). A batch runs the exact call's
// decode, hash and code merge (hg_api.cpp, hg_msgs.cpp), then per check one
// Miller loop on r_i H_i, which also decides whether the check's key lies in
// G2, and per group one Fp12 product, one final exponentiation and the verdict;
// the live members of a group that fails, or that holds a key not proven in
// G2, go through the exact two-pairing check (k_msgs_verify).
#include "bn256_brlc.h"
#include "bn256_sigform.h"
#include "hg_aggregate.h"

namespace {

// the batch on the device; off == nullptr: every check on the context's message
struct BrlcBatch {
  const uint8_t* pool;
  size_t pool_len;
  const uint32_t *off, *len;
  const uint8_t *pks, *sigs;
  size_t n;
  int32_t* codes;
};

void clear_stats(hg_ctx* c) {
  rlc_clear_stats(c);
  c->brlc_non_g2 = 0;
}

// One batch (n <= kSig12MaxN) on stream s with the context's workspaces (the
// streams: MrlcFlow, hg_aggregate.h), the G2 membership of every key out of its
// Miller loop.
int brlc_device_locked(hg_ctx* c, const BrlcBatch& b, const RlcCall& call, hipStream_t s) {
  const bool one = b.off == nullptr;
  if (one && !c->cur.has_msg) {
    c->err = "hg_set_message was not called";
    return HG_ERR_ARG;
  }
  const size_t n = b.n;
  MsgWs& mw = c->msgs;
  // hashedMessage's scalar of the context's message (hg_api.cpp set_message_locked)
  BrlcScalar k1{};
  bool hash_eof = false;
  if (one) {
    uint8_t d[32];
    sha256(c->cur.msg.data(), c->cur.msg.size(), d);
    hash_eof = !hash_scalar(d, k1.w);
  }
  MrlcFlow f(c, call, n, true, s);
  int rc = mrlc_begin(f);
  if (rc) return rc;
  // H_i: the context's for every check, or every check's own message hashed
  if (one)
    launch_brlc_one_message(k1, c->cur.d_h.p, hash_eof ? HG_ERR_HASH_EOF : HG_OK, (int)n, mw.k.p, mw.hcodes.p, mw.h.p,
                            f.hs);
  else {
    launch_hash_scalars(b.pool, b.pool_len, b.off, b.len, (int)n, mw.k.p, mw.hcodes.p, f.hs);
    launch_hash_points(mw.k.p, mw.hcodes.p, (int)n, mw.g1_tab.p, mw.h.p, f.hs);
  }
  rc = mrlc_hashed(f);
  if (rc) return rc;
  // precedence: unmarshal of pk, of sig > hashedMessage's EOF > verdict
  launch_decode_checks(b.pks, b.sigs, (int)n, c->flavor, c->ws.checks.p, b.codes, s);
  rc = mrlc_wait_hashed(f);
  if (rc) return rc;
  launch_merge_hash_codes(mw.hcodes.p, (int)n, b.codes, s);
  rc = mrlc_finish(f, b.codes);
  c->brlc_non_g2 = f.hdr.non_g2;  // zero, as the entry point left it, unless the read-back ran
  return rc;
}

// host pointers in, through the context's staging buffers (as hg_verify_batch, hg_verify_batch_msgs)
int brlc_host_locked(hg_ctx* c, const uint8_t* pool, size_t pool_len, const uint32_t* off, const uint32_t* len,
                     const uint8_t* pks, const uint8_t* sigs, size_t n, const uint64_t* coeffs, const RlcCall& call0,
                     int32_t* codes, int32_t* group_codes, uint32_t* group_live) {
  if (off) {
    int rc = check_ranges(c, call0.who, pool_len, off, len, n);
    if (rc) return rc;
  }
  HG_CHECK(c, hipSetDevice(c->device));
  HG_CHECK(c, c->bytes_a.ensure(n * 128));
  HG_CHECK(c, c->bytes_b.ensure(n * 64));
  HG_CHECK(c, c->ws.codes_c.ensure(n));
  if (coeffs) HG_CHECK(c, c->words.ensure(n));
  hipStream_t s = c->stream;
  Submission sub(c, s);
  HG_CHECK(c, sub.start());
  if (off) {
    int rc = stage_messages(c, pool, pool_len, off, len, n);
    if (rc) return rc;
  }
  HG_CHECK(c, hipMemcpyAsync(c->bytes_a.p, pks, n * 128, hipMemcpyHostToDevice, s));
  HG_CHECK(c, hipMemcpyAsync(c->bytes_b.p, sigs, n * 64, hipMemcpyHostToDevice, s));
  if (coeffs) HG_CHECK(c, hipMemcpyAsync(c->words.p, coeffs, n * 8, hipMemcpyHostToDevice, s));
  RlcCall call = call0;
  call.d_coeffs = coeffs ? c->words.p : nullptr;
  const BrlcBatch b{off ? c->msgs.pool.p : nullptr, pool_len, off ? c->msgs.off.p : nullptr,
                    off ? c->msgs.len.p : nullptr, c->bytes_a.p, c->bytes_b.p, n, c->ws.codes_c.p};
  int rc = brlc_device_locked(c, b, call, s);
  if (rc) return rc;
  HG_CHECK(c, hipMemcpyAsync(codes, b.codes, n * 4, hipMemcpyDeviceToHost, s));
  if (group_codes) {
    rc = rlc_copy_groups(c, rlc_groups(n, call.group), group_codes, group_live, s);
    if (rc) return rc;
  }
  HG_CHECK(c, sub.finish());
  HG_CHECK(c, hipStreamSynchronize(s));
  return HG_OK;
}

// above this the combination's kernels cannot index the batch: the exact call runs
bool too_large(size_t n) { return n > (size_t)kSig12MaxN; }

}  // namespace

extern "C" {

int hg_verify_batch_rlc(hg_ctx* c, const uint8_t* pks, const uint8_t* sigs, size_t n, const uint8_t seed[32],
                        uint32_t group, int32_t* codes) {
  if (!c || !seed || !rlc_group_ok(group) || (n && (!pks || !sigs || !codes)) || n > (size_t)INT32_MAX)
    return HG_ERR_ARG;
  {
    std::lock_guard<std::mutex> g(c->mu);
    clear_stats(c);
    if (n == 0) return HG_OK;
    if (!too_large(n))
      return brlc_host_locked(c, nullptr, 0, nullptr, nullptr, pks, sigs, n, nullptr,
                              RlcCall{"hg_verify_batch_rlc", seed, nullptr, group, true}, codes, nullptr, nullptr);
  }
  return hg_verify_batch(c, pks, sigs, n, codes);
}

int hg_verify_batch_rlc_device(hg_ctx* c, const uint8_t* d_pks, const uint8_t* d_sigs, size_t n,
                               const uint8_t seed[32], uint32_t group, int32_t* d_codes, void* stream) {
  if (!c || !seed || !rlc_group_ok(group) || (n && (!d_pks || !d_sigs || !d_codes)) || n > (size_t)INT32_MAX)
    return HG_ERR_ARG;
  {
    std::lock_guard<std::mutex> g(c->mu);
    clear_stats(c);
    if (n == 0) return HG_OK;
    if (!too_large(n)) {
      HG_CHECK(c, hipSetDevice(c->device));
      hipStream_t s = stream ? (hipStream_t)stream : c->stream;
      return brlc_device_locked(c, BrlcBatch{nullptr, 0, nullptr, nullptr, d_pks, d_sigs, n, d_codes},
                                RlcCall{"hg_verify_batch_rlc_device", seed, nullptr, group, true}, s);
    }
  }
  return hg_verify_batch_device(c, d_pks, d_sigs, n, d_codes, stream);
}

int hg_verify_batch_msgs_rlc(hg_ctx* c, const uint8_t* pool, size_t pool_len, const uint32_t* msg_off,
                             const uint32_t* msg_len, const uint8_t* pks, const uint8_t* sigs, size_t n,
                             const uint8_t seed[32], uint32_t group, int32_t* codes) {
  if (!c || !seed || !rlc_group_ok(group) || (n && (!msg_off || !msg_len || !pks || !sigs || !codes)) ||
      (!pool && pool_len) || n > (size_t)INT32_MAX)
    return HG_ERR_ARG;
  {
    std::lock_guard<std::mutex> g(c->mu);
    clear_stats(c);
    if (n == 0) return HG_OK;
    if (!too_large(n))
      return brlc_host_locked(c, pool, pool_len, msg_off, msg_len, pks, sigs, n, nullptr,
                              RlcCall{"hg_verify_batch_msgs_rlc", seed, nullptr, group, true}, codes, nullptr,
                              nullptr);
  }
  return hg_verify_batch_msgs(c, pool, pool_len, msg_off, msg_len, pks, sigs, n, codes);
}

int hg_verify_batch_msgs_rlc_device(hg_ctx* c, const uint8_t* d_pool, size_t pool_len, const uint32_t* d_msg_off,
                                    const uint32_t* d_msg_len, const uint8_t* d_pks, const uint8_t* d_sigs, size_t n,
                                    const uint8_t seed[32], uint32_t group, int32_t* d_codes, void* stream) {
  if (!c || !seed || !rlc_group_ok(group) || (n && (!d_msg_off || !d_msg_len || !d_pks || !d_sigs || !d_codes)) ||
      (!d_pool && pool_len) || n > (size_t)INT32_MAX)
    return HG_ERR_ARG;
  {
    std::lock_guard<std::mutex> g(c->mu);
    clear_stats(c);
    if (n == 0) return HG_OK;
    if (!too_large(n)) {
      HG_CHECK(c, hipSetDevice(c->device));
      hipStream_t s = stream ? (hipStream_t)stream : c->stream;
      return brlc_device_locked(c, BrlcBatch{d_pool, pool_len, d_msg_off, d_msg_len, d_pks, d_sigs, n, d_codes},
                                RlcCall{"hg_verify_batch_msgs_rlc_device", seed, nullptr, group, true}, s);
    }
  }
  return hg_verify_batch_msgs_device(c, d_pool, pool_len, d_msg_off, d_msg_len, d_pks, d_sigs, n, d_codes, stream);
}

int hg_batch_rlc_stats(hg_ctx* c, uint64_t* groups, uint64_t* groups_failed, uint64_t* rechecked, uint64_t* non_g2) {
  if (!c) return HG_ERR_ARG;
  std::lock_guard<std::mutex> g(c->mu);
  if (groups) *groups = c->rlc_stats[0];
  if (groups_failed) *groups_failed = c->rlc_stats[1];
  if (rechecked) *rechecked = c->rlc_stats[2];
  if (non_g2) *non_g2 = c->brlc_non_g2;
  return HG_OK;
}

int hg_debug_g2_member(hg_ctx* c, const uint8_t* pks, size_t n, uint32_t* flags, int32_t* codes) {
  if (!c || (n && (!pks || !flags || !codes)) || n > (size_t)kSig12MaxN) return HG_ERR_ARG;
  if (n == 0) return HG_OK;
  std::lock_guard<std::mutex> g(c->mu);
  HG_CHECK(c, hipSetDevice(c->device));
  Ws& ws = c->ws;
  MsgWs& mw = c->msgs;
  hipStream_t s = c->stream;
  HG_CHECK(c, c->bytes_a.ensure(n * 128));
  HG_CHECK(c, ws.pts2.ensure(n));
  HG_CHECK(c, ws.pts1.ensure(1));
  HG_CHECK(c, ws.codes_c.ensure(n));
  HG_CHECK(c, ws.checks.ensure(n));
  HG_CHECK(c, mw.f.ensure(n));
  HG_CHECK(c, mw.member.ensure(n));
  Submission sub(c, s);
  HG_CHECK(c, sub.start());
  HG_CHECK(c, hipMemcpyAsync(c->bytes_a.p, pks, n * 128, hipMemcpyHostToDevice, s));
  launch_decode_g2(c->bytes_a.p, (int)n, c->flavor, ws.pts2.p, ws.codes_c.p, s);
  launch_brlc_probe_checks(ws.pts2.p, ws.codes_c.p, (int)n, ws.checks.p, ws.pts1.p, s);
  launch_brlc_miller(ws.checks.p, (int)n, c->d_lines.p, ws.pts1.p, 0, mw.f.p, mw.member.p, s);
  int rc = check_launch(c);
  if (rc) return rc;
  HG_CHECK(c, hipMemcpyAsync(flags, mw.member.p, n * 4, hipMemcpyDeviceToHost, s));
  HG_CHECK(c, hipMemcpyAsync(codes, ws.codes_c.p, n * 4, hipMemcpyDeviceToHost, s));
  HG_CHECK(c, sub.finish());
  HG_CHECK(c, hipStreamSynchronize(s));
  for (size_t i = 0; i < n; i++)
    if (codes[i] != HG_OK) flags[i] = 0;  // no key, no verdict
  return HG_OK;
}

int hg_debug_batch_rlc_groups(hg_ctx* c, const uint8_t* pool, size_t pool_len, const uint32_t* msg_off,
                              const uint32_t* msg_len, const uint8_t* pks, const uint8_t* sigs, size_t n,
                              const uint64_t* coeffs, uint32_t group, int32_t* codes, int32_t* group_codes,
                              uint32_t* group_live) {
  if (!c || !rlc_group_ok(group) || (n && (!pks || !sigs || !coeffs || !codes || !group_codes || !group_live)) ||
      (msg_off == nullptr) != (msg_len == nullptr) || (!pool && pool_len) || too_large(n))
    return HG_ERR_ARG;
  if (n == 0) return HG_OK;
  std::lock_guard<std::mutex> g(c->mu);
  clear_stats(c);
  return brlc_host_locked(c, pool, pool_len, msg_off, msg_len, pks, sigs, n, coeffs,
                          RlcCall{"hg_debug_batch_rlc_groups", nullptr, nullptr, group, false}, codes, group_codes,
                          group_live);
}

}  // extern "C"
