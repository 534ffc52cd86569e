/*
 * handel_gpu.h — C ABI of the MI355X BN256 BLS verification engine.
 *
 * This is the drop-in boundary for Handel's crypto plugin interfaces
 * (crypto.go:14-54: PublicKey / Signature / Constructor / MultiSignature)
 * on the bn256 path. A Go maintainer binds it with cgo;
 * the Python host package handel_amd binds it with ctypes. Plain pointers
 * and sizes only; every entry point is thread-safe per context (a mutex
 * serialises submitters, matching the concurrent Handel instances of
 * simul/node/main.go:63-77). Work submitted on one context runs in
 * submission order even across HIP streams: each asynchronous submission
 * records an event, and the next submission on another stream waits for it,
 * because the submissions share the context's device workspaces.
 *
 * Byte formats are the reference's marshals:
 *   G1 (signature)  64 B  = x || y, 32-byte big-endian affine coords, zeros = infinity
 *   G2 (public key) 128 B = x.x || x.y || y.x || y.y (x = x.x*i + x.y), zeros = infinity
 *   GT              384 B = x/crypto GT.Marshal order
 *   bitsets          willf/bitset words: bit i = word[i >> 6] bit (i & 63)
 */
#ifndef HANDEL_GPU_H
#define HANDEL_GPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Per-check result codes. Each maps 1:1 to the error the reference returns
 * (hg_code_string gives the exact text for the chosen flavor). */
enum hg_code {
  HG_OK = 0,                /* nil */
  HG_ERR_SIG_INVALID = 1,   /* "bn256: signature invalid"            bn256/go/bn256.go:91 */
  HG_ERR_HASH_EOF = 2,      /* "EOF" (hashedMessage, digest >= n)     bn256/go/bn256.go:210-218 */
  HG_ERR_LEVEL = 3,         /* "handel: inconsistent bitset with given level" processing.go:350-352 */
  HG_ERR_PK_UNMARSHAL = 4,  /* "unable to unmarshal"                  bn256/go/bn256.go:117 */
  HG_ERR_SIG_UNMARSHAL = 5, /* "bn256: multisig can't unmarshal"      bn256/go/bn256.go:186 */
  HG_ERR_EMPTY_AGG = 6,     /* empty bitset: the reference dereferences a nil *G2 (panic) */
  HG_ERR_CF_EXCEEDS = 7,    /* cloudflare: "bn256: coordinate exceeds modulus" */
  HG_ERR_CF_MALFORMED = 8,  /* cloudflare: "bn256: malformed point" */
  HG_ERR_CF_SHORT = 9,      /* cloudflare: "bn256: not enough data" */
  /* cloudflare SigBLS.UnmarshalBinary wraps the G1 error (bn256/cf/bn256.go:183-190) */
  HG_ERR_SIG_CF_EXCEEDS = 10,   /* "bn256: multisig can't unmarshal: bn256: coordinate exceeds modulus" */
  HG_ERR_SIG_CF_MALFORMED = 11, /* "bn256: multisig can't unmarshal: bn256: malformed point" */
  HG_ERR_SIG_CF_SHORT = 12,     /* "bn256: multisig can't unmarshal: bn256: not enough data" */
  HG_ERR_MULTI_SIZES = 13,  /* "verify multisignature: inconsistent sizes"  crypto.go:122-124 */
  /* Handel packet intake (hg_parse_packets): handel.go:371-436 validatePacket /
   * parseSignatures, crypto.go:86-110 MultiSignature.Unmarshal, bitset.go:166-177
   * WilffBitSet.UnmarshalBinary over willf/bitset v1.1.10 ReadFrom */
  HG_ERR_PKT_ORIGIN = 20,        /* "packet's origin out of range"              handel.go:374-376 */
  HG_ERR_PKT_LEVEL = 21,         /* "invalid packet's level %d"                 handel.go:378-383 */
  HG_ERR_PKT_EOF = 22,           /* "EOF" (encoding/binary.Read on no bytes)    crypto.go:89, bitset.go:169 */
  HG_ERR_PKT_UNEXPECTED_EOF = 23, /* "unexpected EOF" (binary.Read, short read) */
  HG_ERR_PKT_BITSET_SHORT = 24,  /* "bitset received smaller than expected"     crypto.go:93-96 */
  HG_ERR_PKT_TYPE_MISMATCH = 25, /* "unmarshalling error: type mismatch"        willf ReadFrom */
  HG_ERR_PKT_BITSET_SIZE = 26,   /* "invalid bitset's size for given level"     handel.go:398-401 */
  HG_ERR_PKT_NO_SIG = 27,        /* "no signature in the bitset"                handel.go:402-405 */
  HG_ERR_PKT_ID_RANGE = 28,      /* "globalID outside level's range. id=%d, min=%d, max=%d, level=%d"
                                    partitioner.go:107-119 IndexAtLevel, handel.go:421-425 */
  HG_PKT_NO_IND = 29,            /* not an error: the packet carried no individual signature */
  HG_ERR_ARG = 100,         /* bad argument to this API */
  HG_ERR_DEVICE = 101       /* HIP runtime failure (see hg_last_error) */
};

/* Which upstream library's Unmarshal rules to mirror (simul/lib/config.go:211-225). */
enum hg_flavor {
  HG_FLAVOR_GO = 0, /* golang.org/x/crypto/bn256  ("bn256/go") */
  HG_FLAVOR_CF = 1  /* github.com/cloudflare/bn256 ("bn256", "bn256/cf") */
};

typedef struct hg_ctx hg_ctx;

/* One aggregate-verification request (processing.go:342-368 verifySignature):
 * the level's registry range starts at `offset` (partitioner.go rangeLevel min),
 * `level_size` = max - min, the bitset has `bitlen` bits stored at
 * words[word_offset ...]. bitlen != level_size -> HG_ERR_LEVEL. */
typedef struct {
  uint32_t offset;
  uint32_t bitlen;
  uint32_t level_size;
  uint32_t word_offset;
} hg_request;

/* Context: owns a device, the decoded registry, the hashed message and the
 * precomputed G2Base line table. Replaces bn256.NewConstructor() + the
 * package-level G2Base (bn256/go/bn256.go:22,28-52). */
int hg_create(int device, int flavor, hg_ctx** out);
void hg_destroy(hg_ctx* ctx);
const char* hg_last_error(hg_ctx* ctx);
const char* hg_code_string(int code, int flavor);
/* The error text processing.go's verifySignature returns for a per-request
 * code (processing.go:342-368): VerifySignature's errors (signature invalid,
 * hash EOF) wrapped as "handel: <err>", the level check's own text unwrapped,
 * everything else as hg_code_string. "" for HG_OK. */
const char* hg_processing_error_string(int code, int flavor);
int hg_version(void);
/* The context's flavor (HG_FLAVOR_GO / HG_FLAVOR_CF), -1 for NULL. */
int hg_context_flavor(hg_ctx* ctx);
/* SIMDs of the context's device (compute units x 4): the pairing waves it
 * holds at one wave per SIMD (the padded kernels); 0 on error. */
int hg_context_simds(hg_ctx* ctx);

/* Registry.Identities(...).PublicKey() source: uploads n marshalled G2
 * public keys (PublicKey.UnmarshalBinary, bn256/go/bn256.go:113-120), decoding
 * them on the GPU. codes (nullable, n entries) receives per-key decode codes;
 * returns HG_OK only if every key decoded. On any failure the context is
 * left with NO registry (size 0): every aggregate request then fails its
 * range check instead of reading tables of another registry. */
int hg_registry_load(hg_ctx* ctx, const uint8_t* pks, size_t n, int32_t* codes);
size_t hg_registry_size(hg_ctx* ctx);

/* hashedMessage (bn256/go/bn256.go:210-218) computed once per message and
 * cached on the device. Returns HG_OK or HG_ERR_HASH_EOF. */
int hg_set_message(hg_ctx* ctx, const uint8_t* msg, size_t len);

/* PublicKey.VerifySignature(msg, sig) x n with the message given per call
 * (bn256/go/bn256.go:82-94): hashing (cached when msg equals the context's
 * current message) and verification happen under ONE lock hold, so
 * concurrent callers with different messages cannot interleave. */
int hg_verify_batch_msg(hg_ctx* ctx, const uint8_t* msg, size_t len, const uint8_t* pks, const uint8_t* sigs,
                        size_t n, int32_t* codes);

/* n independent PublicKey.VerifySignature(msg, sig) checks (bn256/go:82-94;
 * simul/p2p/aggregator.go:244). pks: n*128 B, sigs: n*64 B, codes: n. */
int hg_verify_batch(hg_ctx* ctx, const uint8_t* pks, const uint8_t* sigs, size_t n, int32_t* codes);

/* Same, with pks/sigs/codes already resident in device memory; `stream` is a
 * hipStream_t (NULL = the context's stream). Asynchronous on the stream. */
int hg_verify_batch_device(hg_ctx* ctx, const uint8_t* d_pks, const uint8_t* d_sigs, size_t n, int32_t* d_codes,
                           void* stream);

/* n independent PublicKey.VerifySignature(msg_i, sig_i) checks, EACH ON ITS
 * OWN MESSAGE (bn256/go/bn256.go:82-94: the message is an argument of every
 * call). Message i is pool[msg_off[i] .. msg_off[i] + msg_len[i]): any
 * alignment, any length (0 included), messages may share or repeat bytes.
 * hashedMessage (bn256/go/bn256.go:210-218) runs for every check on the device.
 * Per-check precedence is the reference's: the unmarshal error of pk, then of
 * sig (parsed before VerifySignature is called), HG_ERR_HASH_EOF (about 44 %
 * of arbitrary messages: digest 0 or >= Order), then the pairing verdict.
 * Every (off, len) is checked against pool_len before anything is launched:
 * a range past the pool, or pool_len >= 2^32, is HG_ERR_ARG for the call
 * (hg_last_error names the check). n = 0 is HG_OK. The call neither reads nor
 * changes the context's current or cached message, its H, its GT tables or
 * their level, and needs no hg_set_message and no registry. */
int hg_verify_batch_msgs(hg_ctx* ctx, const uint8_t* pool, size_t pool_len, const uint32_t* msg_off,
                         const uint32_t* msg_len, const uint8_t* pks, const uint8_t* sigs, size_t n,
                         int32_t* codes);
/* Same (bn256/go/bn256.go:82-94) with every buffer resident in device memory;
 * `stream` is a hipStream_t (NULL = the context's stream). Asynchronous on the
 * stream, ordered like hg_verify_batch_device. The ranges cannot be checked on
 * the host: a check whose range leaves the pool reads nothing and gets the
 * per-check code HG_ERR_ARG (below the unmarshal errors, like the hash's EOF). */
int hg_verify_batch_msgs_device(hg_ctx* ctx, const uint8_t* d_pool, size_t pool_len, const uint32_t* d_msg_off,
                                const uint32_t* d_msg_len, const uint8_t* d_pks, const uint8_t* d_sigs, size_t n,
                                int32_t* d_codes, void* stream);
/* hashedMessage x n (bn256/go/bn256.go:210-218): h_out[64 i ..] = the G1
 * marshal of H(msg_i), codes[i] = HG_OK; or HG_ERR_HASH_EOF, the 64 bytes then
 * being the generator's marshal (a placeholder). Arguments as
 * hg_verify_batch_msgs. */
int hg_hash_messages(hg_ctx* ctx, const uint8_t* pool, size_t pool_len, const uint32_t* msg_off,
                     const uint32_t* msg_len, size_t n, uint8_t* h_out, int32_t* codes);
/* Probe of the fixed-base multiplication behind hashedMessage's
 * new(bn256.G1).ScalarBaseMult(k) (bn256/go/bn256.go:217): out[64 i ..] = the
 * G1 marshal of k_i * G1 for n scalars of 8 little-endian 32-bit words (any
 * 256-bit value; zeros for a multiple of Order). */
int hg_debug_g1_base_mul(hg_ctx* ctx, const uint32_t* k_words, size_t n, uint8_t* out);
/* hashedMessage's scalar alone, on the host (no context, no GPU): SHA-256 and
 * the crypto/rand.Int(reader, Order) rule (bn256/go/bn256.go:210-216) by the
 * code the device runs. k: 8 little-endian words. HG_OK or HG_ERR_HASH_EOF. */
int hg_debug_hash_scalar(const uint8_t* msg, size_t len, uint32_t k[8]);

/* Verdict bitset of n device-resident codes: bit j of byte b (LSB first) = 1
 * iff check 8b+j returned HG_OK; ceil(n/8) bytes, tail bits 0. Replaces the
 * per-check `err == nil` branch of verifyAndPublish (processing.go:270-287)
 * with the buffer the multi-GPU gather exchanges. Asynchronous on `stream`. */
int hg_pack_verdicts_device(hg_ctx* ctx, const int32_t* d_codes, size_t n, uint8_t* d_bits, void* stream);

/* n aggregate checks against the registry: the Combine fold over the set
 * bits of each request's level range, then VerifySignature
 * (processing.go:342-368; crypto.go:120-137 for a full-registry request).
 * agg_pk_out (nullable): n*128 B marshal of each aggregate public key. */
int hg_verify_aggregate(hg_ctx* ctx, const hg_request* reqs, size_t n, const uint64_t* words, size_t nwords,
                        const uint8_t* sigs, int32_t* codes, uint8_t* agg_pk_out);

/* hg_verify_aggregate with the message given per call: hashing (cached when
 * msg equals the context's current message) and the batch under ONE lock
 * hold, for callers that share a context across messages. */
int hg_verify_aggregate_msg(hg_ctx* ctx, const uint8_t* msg, size_t len, const hg_request* reqs, size_t n,
                            const uint64_t* words, size_t nwords, const uint8_t* sigs, int32_t* codes,
                            uint8_t* agg_pk_out);

/* VerifyMultiSignature (crypto.go:120-137) x n: request i's bitset of
 * bitlens[i] bits at words[word_offsets[i] ...] must span the whole registry
 * (bitlens[i] != registry size -> HG_ERR_MULTI_SIZES, the reference's
 * "verify multisignature: inconsistent sizes"). The reference's "registry
 * returned empty identity" cannot occur: the registry is dense. */
int hg_verify_multisig(hg_ctx* ctx, const uint32_t* bitlens, const uint32_t* word_offsets, size_t n,
                       const uint64_t* words, size_t nwords, const uint8_t* sigs, int32_t* codes);

/* n aggregate checks against the registry, EACH ON ITS OWN MESSAGE: request i
 * is hg_verify_aggregate's request, verified against hashedMessage(msg_i)
 * (processing.go:342-368 verifySignature; crypto.go:120-137
 * VerifyMultiSignature(msg, ms, reg, cons) takes the message per call: a node
 * catching up on many rounds, a monitor, a bridge). Message i is
 * pool[msg_off[i] .. msg_off[i] + msg_len[i]) as in hg_verify_batch_msgs: any
 * alignment, any length (0 included), ranges may repeat. Per-request
 * precedence: the signature's unmarshal error, HG_ERR_LEVEL, HG_ERR_HASH_EOF,
 * HG_ERR_EMPTY_AGG, the pairing verdict. agg_pk_out (nullable) as
 * hg_verify_aggregate: the marshal of the aggregate key, zeros for a level
 * error or an empty bitset; it does not depend on the message. Every message
 * range is checked against pool_len (which must be below 2^32) and every
 * request's word range against nwords before anything is launched: a violation
 * is HG_ERR_ARG for the call and hg_last_error names the request. n = 0 is
 * HG_OK. GT tables hold e(H, pk_i) for one H and cannot serve this call: every
 * batch folds the keys in G2 and runs the two-pairing check with H per request
 * (the path that also serves a go-flavor registry with keys outside G2), the
 * hash on a side stream beside the fold unless hg_set_fold_overlap(ctx, 0).
 * The pairing always runs in its one-kernel form, whatever hg_set_verify_split
 * says. The call needs a registry but no hg_set_message; it neither reads nor
 * changes the context's current or cached message, their H, the GT tables,
 * their level or the request count of the table policy. */
int hg_verify_aggregate_msgs(hg_ctx* ctx, const uint8_t* pool, size_t pool_len, const uint32_t* msg_off,
                             const uint32_t* msg_len, const hg_request* reqs, size_t n, const uint64_t* words,
                             size_t nwords, const uint8_t* sigs, int32_t* codes, uint8_t* agg_pk_out);
/* Same (processing.go:342-368, crypto.go:120-137) with every buffer resident in
 * device memory; `stream` is a hipStream_t (NULL = the context's stream).
 * Asynchronous on the stream, ordered like hg_verify_aggregate_device. The
 * ranges cannot be checked on the host: a request whose message range leaves
 * the pool reads nothing and gets the per-request code HG_ERR_ARG, in the hash
 * code's place in the precedence (below the unmarshal and level errors). */
int hg_verify_aggregate_msgs_device(hg_ctx* ctx, const uint8_t* d_pool, size_t pool_len, const uint32_t* d_msg_off,
                                    const uint32_t* d_msg_len, const hg_request* d_reqs, size_t n,
                                    const uint64_t* d_words, const uint8_t* d_sigs, int32_t* d_codes,
                                    uint8_t* d_agg_pk_out, void* stream);
/* VerifyMultiSignature(msg_i, ms_i, reg, cons) x n (crypto.go:120-137), each
 * multisignature on its own message: hg_verify_multisig's requests with
 * hg_verify_aggregate_msgs's messages and precedence, HG_ERR_MULTI_SIZES
 * standing where the aggregate form gives HG_ERR_LEVEL. */
int hg_verify_multisig_msgs(hg_ctx* ctx, const uint8_t* pool, size_t pool_len, const uint32_t* msg_off,
                            const uint32_t* msg_len, const uint32_t* bitlens, const uint32_t* word_offsets, size_t n,
                            const uint64_t* words, size_t nwords, const uint8_t* sigs, int32_t* codes);

/* Builds the per-(message, registry) tables of aggregate verification now:
 * e(H, pk_i) for every registry key and the GT products of every 8-key and
 * 16-key window subset and aligned block (bilinearity: e(H, sum pk_i) =
 * prod e(H, pk_i); the aggregate check is then a GT fold plus ONE pairing per
 * request). For serving a stream of batches (≈ 15 ms and ≈ 2 MB of HBM per
 * key; registries above 16384 keys get the 8-key tables only). Without it the
 * context builds the 8-key level after 16384 requests of one message (≈ 3 ms
 * for 4000 keys) and the 16-key level after 2^20, verifying earlier requests
 * with the G2 point fold. Tables follow the context's current message and
 * registry. HG_OK; HG_ERR_HASH_EOF (message cannot be hashed: nothing to
 * build); HG_ERR_ARG without a message or registry. Synchronous. */
int hg_prepare_aggregate(hg_ctx* ctx);
/* hg_set_message + hg_prepare_aggregate under ONE lock hold, so a concurrent
 * caller with another message cannot take the tables in between (the Go
 * PrepareAggregate, bn256/go/bn256.go:210-218: H is fixed per Handel run). */
int hg_prepare_aggregate_msg(hg_ctx* ctx, const uint8_t* msg, size_t len);
/* The table level aggregate requests currently run at: 0 = G2 point fold and
 * two-pairing check, 1 = GT fold over 8-key windows, 2 = over 16-key windows.
 * The tables are a cache: a level the device cannot hold (or that exceeds the
 * table budget) is skipped and requests run at the level below, down to 0.
 * A go-flavor registry holding a key outside G2 stays at 0 (see
 * hg_registry_non_g2). */
int hg_aggregate_tables(hg_ctx* ctx);
/* 1 when the level-2 tables are kept in torus form (the fold then takes two
 * Fp6 products per term instead of an Fp12 product; same verdicts), else 0:
 * below level 2, with HG_GT_TORUS=0 in the environment, or for a registry in
 * which some window subset or aligned block of keys sums to zero (such a
 * value has no torus form; the tables then stay as they were). */
int hg_aggregate_tables_torus(hg_ctx* ctx);
/* Pins the table level of this context's aggregate submissions (0..2, capped
 * as above) or, with -1, returns them to the volume policy. New contexts take
 * HG_GT_LEVEL / HG_AGG_PATH=g2 (= 0) from the environment, else -1. */
int hg_set_aggregate_level(hg_ctx* ctx, int level);
/* GT path: run the fold on a side stream beside the pairing kernel (1, the
 * default; HG_GT_OVERLAP=0 makes 0 the default of new contexts) or before it
 * (0). Same verdicts; the overlap hides the fold when one batch is in flight,
 * several contexts each with a batch in flight may prefer 0. */
int hg_set_fold_overlap(hg_ctx* ctx, int on);
/* Config 2 (hg_verify_batch*): the check's form. 0 (the default; HG_VERIFY_SPLIT
 * gives new contexts its value): one kernel per batch, the faster form when a
 * batch runs alone. 1: the split form — the Miller loop on a compact team
 * region, then the 12-lane final exponentiation with batched inversions — for
 * several contexts each keeping a batch in flight, whose waves then share the
 * SIMDs. Same verdicts (PublicKey.VerifySignature, bn256/go/bn256.go:82-94). */
int hg_set_verify_split(hg_ctx* ctx, int on);
/* Upper bound in bytes for this context's GT tables (default: unlimited, the
 * device's free memory decides). Processes sharing one GPU (simul's P
 * processes x k instances, simul/node/main.go:63-131) give each context a
 * share; level-2 tables take ~1.97 MB per key, level 1 ~15 kB per key. */
int hg_set_table_budget(hg_ctx* ctx, size_t bytes);
/* Keys of the loaded registry that lie on the twist but outside the order-n
 * subgroup G2. x/crypto's G2.Unmarshal accepts them (bn256/go/bn256.go:113-120;
 * cloudflare rejects them at load). The GT product e(H, pk_1)...e(H, pk_k)
 * equals the reference's e(H, pk_1 + ... + pk_k) only on G2, so a registry
 * with such keys is served by the G2 fold and the two-pairing check. */
size_t hg_registry_non_g2(hg_ctx* ctx);

/* Device-resident variant (reqs, words, sigs, codes, agg out on the device). */
int hg_verify_aggregate_device(hg_ctx* ctx, const hg_request* d_reqs, size_t n, const uint64_t* d_words,
                               const uint8_t* d_sigs, int32_t* d_codes, uint8_t* d_agg_pk_out, void* stream);

/* hg_verify_aggregate_device (verdicts only) plus the verdict bitset of the
 * codes (hg_pack_verdicts_device's layout, ceil(n/8) bytes) in the same
 * submission: the serving step's codes -> bitset launch folds into the
 * comparison (processing.go:270-287's err == nil branch, batched). */
int hg_verify_aggregate_device_bits(hg_ctx* ctx, const hg_request* d_reqs, size_t n, const uint64_t* d_words,
                                    const uint8_t* d_sigs, int32_t* d_codes, uint8_t* d_bits, void* stream);

/* ---------------------------------------------------------------- random linear combination
 * hg_verify_aggregate with the pairings of `group` checks at a time replaced by
 * one. For the checks i of a group, with F_i = prod e(H, pk_j) over check i's
 * set keys (the GT fold's value),
 *     e(sum r_i sig_i, G2Base) == prod F_i^(r_i)
 * holds when every check holds, and with probability <= 2^-64 over the
 * coefficients when one does not. Codes are hg_verify_aggregate's, check for
 * check (processing.go:342-368 verifySignature), except that an invalid
 * signature is accepted with probability <= 2^-64 over `seed`.
 * seed: 32 bytes the sender of the signatures cannot predict (fresh randomness
 * per call); r_i = the first 8 bytes, little-endian, of
 * SHA-256("hg-rlc-v1" || seed || LE64(i)), 0 replaced by 1. group: 1..4096;
 * groups are the index ranges [g group, (g + 1) group).
 * The combination runs exactly when hg_verify_aggregate_device would take a GT
 * flow (a message is set, tables at level 1 or 2: every registry key is then
 * proven to lie in G2); otherwise the call is the exact path and hg_rlc_stats
 * reports 0 groups. Checks the prologue and the fold already decided (unmarshal,
 * level, empty aggregate) keep their code and join no group; a group without a
 * live member is skipped. The live members of a group whose combined check
 * fails are verified again one by one, so every code is exact. Sizing that
 * launch needs the failed groups' member count on the host: each call that runs
 * the combination synchronises its stream once and reads 16 bytes back (the
 * count and the statistics), the _device form included. group == 0,
 * group > 4096 or a NULL seed: HG_ERR_ARG. n = 0: HG_OK. */
int hg_verify_aggregate_rlc(hg_ctx* ctx, const hg_request* reqs, size_t n, const uint64_t* words, size_t nwords,
                            const uint8_t* sigs, const uint8_t seed[32], uint32_t group, int32_t* codes);
int hg_verify_aggregate_rlc_device(hg_ctx* ctx, const hg_request* d_reqs, size_t n, const uint64_t* d_words,
                                   const uint8_t* d_sigs, const uint8_t seed[32], uint32_t group, int32_t* d_codes,
                                   void* stream);
/* last RLC call on this context: groups checked, groups that failed, checks re-verified one by one */
int hg_rlc_stats(hg_ctx* ctx, uint64_t* groups, uint64_t* groups_failed, uint64_t* rechecked);
/* r_i for i = first .. first+n-1, on the host, by the code the device runs (no GPU) */
int hg_debug_rlc_coeffs(const uint8_t seed[32], uint64_t first, size_t n, uint64_t* out);
/* probes with caller-given coefficients (tests only; never use for verification).
 * hg_debug_rlc_g1: out64_per_group[64 g ..] = the G1 marshal of sum coeffs[i] sigs[i]
 * over group g's signatures (zeros for infinity), ceil(n / group) groups; a
 * signature that does not unmarshal is left out.
 * hg_debug_rlc_groups: everything up to the group comparison, no recheck:
 * codes[n] = the prologue's and the fold's codes, group_codes[g] = HG_OK or
 * HG_ERR_SIG_INVALID, group_live[g] = group g's live members. HG_ERR_ARG when
 * the context would not run the combination (no GT tables). */
int hg_debug_rlc_g1(hg_ctx* ctx, const uint8_t* sigs, size_t n, const uint64_t* coeffs, uint32_t group,
                    uint8_t* out64_per_group);
int hg_debug_rlc_groups(hg_ctx* ctx, const hg_request* reqs, size_t n, const uint64_t* words, size_t nwords,
                        const uint8_t* sigs, const uint64_t* coeffs, uint32_t group, int32_t* codes,
                        int32_t* group_codes, uint32_t* group_live);

/* ---------------------------------------------------------------- ... with a message per request
 * hg_verify_aggregate_msgs (verdicts only: no agg_pk_out, the exact call serves
 * callers who want the keys) with the final exponentiations of `group`
 * requests at a time replaced by one (processing.go:342-368 verifySignature;
 * crypto.go:120-137 VerifyMultiSignature(msg, ms, reg, cons) with the message
 * per call). GT tables hold e(H, pk_i) for one H and cannot help here; for the
 * live requests i of a group, with agg_i the aggregate key of request i,
 *     prod e(r_i H_i, agg_i) * e(-sum r_i sig_i, G2Base) == 1
 * holds when every check holds, and with probability <= 2^-64 over the
 * coefficients when one does not: a request costs one Miller loop and one Fp12
 * product, a group one final exponentiation. Messages, argument rules and
 * per-request precedence are hg_verify_aggregate_msgs*'s; seed, r_i and group
 * are hg_verify_aggregate_rlc's (NULL seed, group == 0 or group > 4096:
 * HG_ERR_ARG; n = 0: HG_OK). A request is live when everything decided before
 * the pairing left it HG_OK (unmarshal, level, hash, empty aggregate); an
 * infinity signature on a non-empty set is live and fails its group. The live
 * members of a group that fails are verified again one by one on the exact
 * call's path, so every code is hg_verify_aggregate_msgs's, except that an
 * invalid signature is accepted with probability <= 2^-64 over `seed`.
 * The combination runs when every registry key is proven to lie in G2
 * (hg_registry_non_g2 == 0; the call waits for a membership check still
 * running); otherwise, and above 2^28 requests, the call is
 * hg_verify_aggregate_msgs_device's path as it stands and hg_rlc_stats reports
 * zeros. Like the exact calls these need a registry and no hg_set_message, and
 * neither read nor change the context's messages, their H, the GT tables, their
 * level or the request count of the table policy. Each call that runs the
 * combination synchronises its stream once and reads 16 bytes back, the
 * _device form included. hg_rlc_stats reports on these calls too. */
int hg_verify_aggregate_msgs_rlc(hg_ctx* ctx, const uint8_t* pool, size_t pool_len, const uint32_t* msg_off,
                                 const uint32_t* msg_len, const hg_request* reqs, size_t n, const uint64_t* words,
                                 size_t nwords, const uint8_t* sigs, const uint8_t seed[32], uint32_t group,
                                 int32_t* codes);
int hg_verify_aggregate_msgs_rlc_device(hg_ctx* ctx, const uint8_t* d_pool, size_t pool_len, const uint32_t* d_msg_off,
                                        const uint32_t* d_msg_len, const hg_request* d_reqs, size_t n,
                                        const uint64_t* d_words, const uint8_t* d_sigs, const uint8_t seed[32],
                                        uint32_t group, int32_t* d_codes, void* stream);
/* VerifyMultiSignature(msg_i, ms_i, reg, cons) x n (crypto.go:120-137) in the
 * combined form: hg_verify_multisig_msgs's requests and its rename of
 * HG_ERR_LEVEL to HG_ERR_MULTI_SIZES (processing.go:342-368 for the rest). */
int hg_verify_multisig_msgs_rlc(hg_ctx* ctx, const uint8_t* pool, size_t pool_len, const uint32_t* msg_off,
                                const uint32_t* msg_len, const uint32_t* bitlens, const uint32_t* word_offsets,
                                size_t n, const uint64_t* words, size_t nwords, const uint8_t* sigs,
                                const uint8_t seed[32], uint32_t group, int32_t* codes);
/* probes with caller-given coefficients (tests only; never use for verification).
 * hg_debug_msgs_rlc_groups: everything up to the group verdicts, no recheck:
 * codes[n] = what is decided before the pairing, group_codes[g] = HG_OK or
 * HG_ERR_SIG_INVALID, group_live[g] = group g's live members. HG_ERR_ARG when
 * the context would not run the combination.
 * hg_debug_msgs_rlc_points: out[64 i ..] = the G1 marshal of
 * coeffs[i] hashedMessage(msg_i); zeros where the message cannot be hashed. */
int hg_debug_msgs_rlc_groups(hg_ctx* ctx, const uint8_t* pool, size_t pool_len, const uint32_t* msg_off,
                             const uint32_t* msg_len, const hg_request* reqs, size_t n, const uint64_t* words,
                             size_t nwords, const uint8_t* sigs, const uint64_t* coeffs, uint32_t group,
                             int32_t* codes, int32_t* group_codes, uint32_t* group_live);
int hg_debug_msgs_rlc_points(hg_ctx* ctx, const uint8_t* pool, size_t pool_len, const uint32_t* msg_off,
                             const uint32_t* msg_len, const uint64_t* coeffs, size_t n, uint8_t* out);

/* ---------------------------------------------------------------- ... of independent checks on arbitrary keys
 * hg_verify_batch and hg_verify_batch_msgs (n independent
 * PublicKey.VerifySignature checks, bn256/go/bn256.go:82-94;
 * simul/p2p/aggregator.go:244) with the final exponentiations of `group` checks
 * at a time replaced by one. For the live checks i of a group, with H_i the
 * context's H or the check's own,
 *     prod e(r_i H_i, pk_i) * e(-sum r_i sig_i, G2Base) == 1
 * holds when every check holds, and with probability <= 2^-64 over the
 * coefficients when one does not, provided every pk_i lies in G2. The keys are
 * arbitrary points of the twist (G2.Unmarshal, bn256/go/bn256.go:113-120), so
 * each check's Miller loop also decides whether its key lies in G2 (the loop
 * ends on [6u+2]Q + psi(Q) - psi^2(Q), which equals -psi^3(Q) exactly on G2;
 * DESIGN.md §3n): a group that holds a live check whose key is not proven in G2
 * counts as failed whatever its product. A check costs one Miller loop and one
 * Fp12 product, a group one final exponentiation.
 * hg_verify_batch_rlc* run on the context's current message, as
 * hg_verify_batch (HG_ERR_ARG without hg_set_message); the codes are
 * hg_verify_batch's, check for check. hg_verify_batch_msgs_rlc*: messages,
 * argument rules, range checks and per-check precedence are
 * hg_verify_batch_msgs*'s. seed, r_i and group are hg_verify_aggregate_rlc's
 * (NULL seed, group == 0 or group > 4096: HG_ERR_ARG; n = 0: HG_OK). A check
 * is live when everything decided before the pairing left it HG_OK (unmarshal,
 * cf's subgroup check, hash); an infinity signature is live, a key at infinity
 * is live and counts as a member. The live members of a group that fails are
 * verified again one by one with the exact two-pairing check, so every code is
 * the exact call's, except that an invalid signature is accepted with
 * probability <= 2^-64 over `seed`. Above 2^28 checks the call is the exact
 * call as it stands and the statistics are zeros. Each call that runs the
 * combination synchronises its stream once and reads 16 bytes back, the _device
 * forms included. */
int hg_verify_batch_rlc(hg_ctx* ctx, const uint8_t* pks, const uint8_t* sigs, size_t n, const uint8_t seed[32],
                        uint32_t group, int32_t* codes);
int hg_verify_batch_rlc_device(hg_ctx* ctx, const uint8_t* d_pks, const uint8_t* d_sigs, size_t n,
                               const uint8_t seed[32], uint32_t group, int32_t* d_codes, void* stream);
int hg_verify_batch_msgs_rlc(hg_ctx* ctx, const uint8_t* pool, size_t pool_len, const uint32_t* msg_off,
                             const uint32_t* msg_len, const uint8_t* pks, const uint8_t* sigs, size_t n,
                             const uint8_t seed[32], uint32_t group, int32_t* codes);
int hg_verify_batch_msgs_rlc_device(hg_ctx* ctx, const uint8_t* d_pool, size_t pool_len, const uint32_t* d_msg_off,
                                    const uint32_t* d_msg_len, const uint8_t* d_pks, const uint8_t* d_sigs, size_t n,
                                    const uint8_t seed[32], uint32_t group, int32_t* d_codes, void* stream);
/* last hg_verify_batch*_rlc* call on this context: groups, groups_failed and
 * rechecked as hg_rlc_stats (which reports on these calls too); non_g2 = the
 * live checks whose key was not proven to lie in G2 (each fails its group). */
int hg_batch_rlc_stats(hg_ctx* ctx, uint64_t* groups, uint64_t* groups_failed, uint64_t* rechecked,
                       uint64_t* non_g2);
/* probes (tests only; never use for verification).
 * hg_debug_g2_member: the keys decoded by the context's flavor
 * (PublicKey.UnmarshalBinary, bn256/go/bn256.go:113-120; codes[i]), each run
 * through the membership Miller loop with H the G1 generator: flags[i] = 1 for
 * a key in G2 or at infinity, 0 for any other key and where the key does not
 * decode.
 * hg_debug_batch_rlc_groups: caller-given coefficients, everything up to the
 * group verdicts, no recheck: codes[n] = what is decided before the pairing,
 * group_codes[g] = HG_OK or HG_ERR_SIG_INVALID, group_live[g] = group g's live
 * members. msg_off == msg_len == NULL: every check on the context's message. */
int hg_debug_g2_member(hg_ctx* ctx, const uint8_t* pks, size_t n, uint32_t* flags, int32_t* codes);
int hg_debug_batch_rlc_groups(hg_ctx* ctx, const uint8_t* pool, size_t pool_len, const uint32_t* msg_off,
                              const uint32_t* msg_len, const uint8_t* pks, const uint8_t* sigs, size_t n,
                              const uint64_t* coeffs, uint32_t group, int32_t* codes, int32_t* group_codes,
                              uint32_t* group_live);

/* Batched PublicKey.Combine fold only: n requests -> n*128 B aggregate keys
 * (bn256/go/bn256.go:97-105). codes: HG_OK, HG_ERR_LEVEL or HG_ERR_EMPTY_AGG. */
int hg_aggregate_pk(hg_ctx* ctx, const hg_request* reqs, size_t n, const uint64_t* words, size_t nwords,
                    uint8_t* agg_pk_out, int32_t* codes);

/* Batched SigBLS.Combine (bn256/go/bn256.go:192-200): out[i] = a[i] + b[i]. */
int hg_combine_g1(hg_ctx* ctx, const uint8_t* a, const uint8_t* b, size_t n, uint8_t* out, int32_t* codes);

/* Batched PublicKey.Combine on marshalled keys (bn256/go/bn256.go:97-105):
 * out[i] = a[i] + b[i] in G2 (n*128 B each). */
int hg_combine_g2(hg_ctx* ctx, const uint8_t* a, const uint8_t* b, size_t n, uint8_t* out, int32_t* codes);

/* bn256.Pair(g1[i], g2[i]).Marshal() — the GT values the reference compares
 * in VerifySignature (bn256/go/bn256.go:88-89); parity probe. */
int hg_pair(hg_ctx* ctx, const uint8_t* g1s, const uint8_t* g2s, size_t n, uint8_t* gt_out, int32_t* codes);

/* Batch keygen / signing for fixtures and simulation start-up:
 * NewKeyPair's pk = k * G2 (bn256/go/bn256.go:129-142) and Sign's
 * sig = k * H(msg) (bn256/go/bn256.go:146-154) for n big-endian 32-byte
 * scalars. hg_sign needs hg_set_message first (returns HG_ERR_HASH_EOF when
 * the message cannot be hashed). */
int hg_keygen(hg_ctx* ctx, const uint8_t* scalars_be, size_t n, uint8_t* pks_out);
int hg_sign(hg_ctx* ctx, const uint8_t* scalars_be, size_t n, uint8_t* sigs_out);
/* SecretKey.Sign(msg) x n with the message given per call (one lock hold,
 * like hg_verify_batch_msg). */
int hg_sign_msg(hg_ctx* ctx, const uint8_t* msg, size_t len, const uint8_t* scalars_be, size_t n,
                uint8_t* sigs_out);

/* Self test of the field multiplier: out = a*b mod p on plain 256-bit
 * little-endian 32-bit words (8 per element). */
int hg_debug_fp_mul(hg_ctx* ctx, const uint32_t* a, const uint32_t* b, size_t n, uint32_t* out);

/* Measurement hooks: when enabled, device work is bracketed by HIP events on
 * the stream it runs on, per phase: HG_PHASE_VERIFY = every launch of the
 * pairing-check kernel, HG_PHASE_AGGREGATE = the Combine fold of an aggregate
 * submission (plan, order, fold, finish), HG_PHASE_SUBMIT = a whole
 * verification submission (decode/aggregate + check). hg_timing_read_phase
 * returns (and clears) the summed time and the count of bracketed intervals;
 * hg_timing_read is hg_timing_read_phase(HG_PHASE_VERIFY). */
enum hg_phase { HG_PHASE_VERIFY = 0, HG_PHASE_AGGREGATE = 1, HG_PHASE_SUBMIT = 2, HG_NUM_PHASES = 3 };
int hg_timing_enable(hg_ctx* ctx, int on);
int hg_timing_read(hg_ctx* ctx, double* total_ms, int* launches);
int hg_timing_read_phase(hg_ctx* ctx, int phase, double* total_ms, int* launches);

/* Parity probe of the team Fp12 building blocks: elements are 384-byte GT
 * marshals. op: 0 a*b, 1 a^2, 2 cyclotomic a^2, 3 a^p, 4 a^(p^2), 5 a^-1,
 * 6 conj(a), 7 a^u, 8 final exponentiation, 10 cyclotomic a^2 by the
 * canonical squaring program (9 is retired). Bits 8.. of op: repetitions.
 * Any other op: HG_ERR_ARG. */
int hg_debug_fp12(hg_ctx* ctx, int op, const uint8_t* a, const uint8_t* b, size_t n, uint8_t* out);

/* Probe of ONE generated team-program instance (bn256_xtab.h), for the
 * limb-for-limb comparison with the generator's model: inst is the
 * instance's position in tools/gen_g2_schedule.py's ALL_INSTANCES. in and out
 * hold n team regions of *region_elems elements of ten 32-bit limbs each,
 * taken and returned as they are (no Montgomery conversion, no reduction, no
 * marshal order): a region is copied into the team's LDS, the instance runs
 * once on the team of the production kernel of its layout, and the whole
 * region comes back. form 0: one-wave teams; form 1: the 2-wave split teams,
 * layout-S instances only. An inst out of range, another form, or form 1 on
 * another layout: HG_ERR_ARG, nothing runs, out and region_elems untouched.
 * n = 0 only reports region_elems (may be NULL otherwise). n <= 2^20. */
int hg_debug_xinst(hg_ctx* ctx, int inst, int form, const uint32_t* in, size_t n, uint32_t* out, int* region_elems);

/* Probe of ONE per-thread primitive of bn256_fp.h / bn256_curve.h, for the
 * bit-exact comparison with an integer reference: one thread per case, the
 * production function itself. in and out hold n cases of *in_words and
 * *out_words 32-bit words. An Fp element is ten words, the 26-bit limbs Fp::l
 * as they are (Montgomery form, R = 2^286; no conversion, no reduction), an
 * Fp2 is x then y, a Jacobian point x, y, z, an affine point x, y. Operands
 * are canonical, in [0, p), unless stated. op (words in -> out):
 *    0 fp_add(a, b)        1 fp_sub(a, b)       2 fp_neg(a)      3 fp_dbl(a)
 *    4 fp_mul3(a)          5 fp_mul(a, b)       6 fp_sqr(a)      7 fp_inv(a), 0 -> 0
 *    8 fp_neg_loose(a): normalised limbs of p - a, so p for a = 0
 *    9 fp_add_loose(a, b): the limb-wise sums
 *   10 fp_to_mont(words_to_limbs(w)): 8 LE words of any integer < 2^256 -> 10
 *   11 limbs_to_words(fp_from_mont(a)): 10 -> 8 LE words
 *   12 fp_from_be: word 0 = a byte offset k in 0..3, words 1..9 = a 36-byte
 *      buffer holding 32 big-endian bytes (any integer < 2^256) at byte k; k = 0
 *      takes be_to_words' dword path, the others its byte path. 10 -> 12: the
 *      element, ge (the integer is >= p), nz (some byte is nonzero)
 *   13 fp_to_be(a): 10 -> 8 words holding the 32 big-endian bytes
 *   14 f2_mul(a, b)  15 f2_sqr(a)  16 f2_muls(a, s in Fp)  17 f2_mul_xi(a)
 *   18 f2_inv(a), 0 -> 0           19 f2_sub(a, b)  20 f2_neg(a)  21 f2_conj(a)
 *   22 g1_double(P)  23 g1_add(P, Q)  24 g1_madd(P, affine Q)  25 g1_on_curve(x, y) -> 1 word
 *   26 g1_affine(P), infinity -> (0, 0)
 *   27 g2_double(P)  28 g2_add(P, Q)  29 g2_madd(P, affine Q)  30 g2_add_affine(P, affine Q)
 *   31 g2_on_curve(x, y) -> 1 word    32 g2_affine(P), infinity -> (0, 0)
 * Jacobian operands: coordinates in [0, p), on the curve (X, Y, Z with
 * Y^2 = X^3 + b Z^6) or at infinity (Z = 0, X and Y anything); the affine
 * operand of 24, 29, 30 is a finite point of the curve; 25, 26, 31, 32 take
 * any canonical coordinates. An unknown op, NULL in or out with n > 0, or
 * n > 2^20: HG_ERR_ARG, nothing runs, out and the word counts untouched.
 * n = 0 only reports the word counts (either may be NULL). */
int hg_debug_field(hg_ctx* ctx, int op, const uint32_t* in, size_t n, uint32_t* out, int* in_words, int* out_words);

/* Read-back of the GT path's key side, for the value-level comparison with
 * g^(sum of k_i): the current message's table set as the kernels left it and
 * the fold's values before any pairing. Nothing here converts or reduces: an
 * entry is the 120 words Gt::w (element 2k + c of coefficient k of w, c = 0: x;
 * ten 26-bit limbs of the Montgomery representative; a torus entry holds alpha
 * in elements 0..5 and zeros after). All three: HG_ERR_ARG without a built
 * table set (hg_aggregate_tables() == 0), out untouched.
 *
 * hg_debug_gt_layout: HG_GT_LAYOUT_WORDS ints: built level, torus flag, nreg,
 * 8-key windows, 16-key windows, highest block level K, then base[k] and
 * count[k] for k = 0..23 (block (k, j), 4 <= k <= K, is entry base[k] + j of
 * the block table; zero outside 4..K). */
#define HG_GT_LAYOUT_WORDS 54
#define HG_GT_TABLE_KEYS 0   /* nreg entries */
#define HG_GT_TABLE_WIN8 1   /* 256 per 8-key window */
#define HG_GT_TABLE_WIN16 2  /* 65536 per 16-key window (level 2) */
#define HG_GT_TABLE_BLOCKS 3 /* the sum of count[k] */
int hg_debug_gt_layout(hg_ctx* ctx, int32_t* out);
/* count entries from `first` of one table into out (120 words each): a
 * synchronous device-to-host copy. HG_ERR_ARG for an unknown or unbuilt table
 * or a range past its end. */
int hg_debug_gt_entries(hg_ctx* ctx, int table, size_t first, size_t count, uint32_t* out);
/* The fold alone over the tables as built (the window width and the form an
 * aggregate submission would use), in `chunk` (1..64) terms per chunk, with
 * workspaces of its own sized for that chunk: the level check, the plan, the
 * chunk products and the combine; no pairing, no comparison. y: n x 120 words,
 * the fold's Y = conj(e(H, aggregate key)) (Fp12 form) or X with
 * X/conj(X) = Y (torus form), zeros where codes[r] is not HG_OK; codes: HG_OK,
 * HG_ERR_LEVEL or HG_ERR_EMPTY_AGG. HG_ERR_ARG also for n = 0, n > 2^20, a
 * chunk outside 1..64 or a request whose words leave the bitset. */
int hg_debug_gt_fold(hg_ctx* ctx, const hg_request* reqs, size_t n, const uint64_t* words, size_t nwords, int chunk,
                     uint32_t* y, int32_t* codes);

/* Kernel probe of the GT path's signature side (bench.py per-kernel
 * roofline, the GPU suite's cross-kernel check): d_fe[r] (480 bytes, the
 * engine's internal GT layout) = FE(Miller(G2Base at -sig_r)) for the n
 * 64-byte signature marshals at d_sigs (context flavor), computed by kernel
 * (the numbers are SigForm's, handel_amd/csrc/bn256_sigform.h)
 * 0: k_verify_sig padded (one wave per SIMD), 1: k_verify_sig unpadded,
 * 2: k_sig_scalars + k_sig_lines + k_verify_sig12 padded, 3: the same
 * unpadded (what a lane in flight runs: since r06 split into k_sig12_miller,
 * k_sig12_ninv, k_sig12_fe unless HG_SIG12_SPLIT=0), 4: k_verify_sig_split<2> (two
 * waves per check: the padded latency form for n <= 2048). Enqueued on `stream` (NULL: the
 * context's), ordered like every submission of the context. Replaces no
 * reference interface: the product paths choose the kernel themselves. */
int hg_sig_pairing_device(hg_ctx* ctx, const uint8_t* d_sigs, size_t n, uint8_t* d_fe, int kernel, void* stream);

/* Diagnostic builds only (-DHG_DIAG, tools/diag.py): per-block s_memtime
 * phase counters of the last pairing-check launch; HG_ERR_ARG otherwise. */
int hg_diag_read(hg_ctx* ctx, uint64_t* out, size_t n);

/* Wait for all work submitted on the context's stream. */
int hg_sync(hg_ctx* ctx);

/* Device memory held by the context (registry, its sums, GT tables,
 * workspaces), in bytes: the HBM one simul process's verifier costs. */
size_t hg_context_bytes(hg_ctx* ctx);

/* ---------------------------------------------------------------- packet intake
 * Handel.NewPacket's parse step for a batch of received packets (handel.go:
 * 127-152 -> validatePacket :371-385 -> parseSignatures :389-436): the origin
 * and level checks against the RECEIVING instance's partitioner
 * (partitioner.go:95-178), MultiSignature.Unmarshal of the wire bytes
 * (crypto.go:86-110: u16 BE blob length, the WilffBitSet blob = u16 BE bit
 * length + willf's u64 BE length and u64 BE words, then the signature
 * marshal), the bit-length and empty-bitset checks, and the optional
 * individual signature with its IndexAtLevel check. The output is the
 * verification requests processing.go's verifySignature runs on
 * (hg_verify_aggregate*), already in HBM for the device variant. */
typedef struct {
  int32_t origin;     /* Packet.Origin (net.go:36) */
  uint32_t receiver;  /* id of the Handel instance that received it (its partitioner) */
  uint32_t level;     /* Packet.Level (net.go:39; a byte on the wire) */
  uint32_t flags;     /* HG_PKT_HAS_IND: Packet.IndividualSig is non-nil */
  uint32_t ms_off, ms_len;   /* Packet.MultiSig = pool[ms_off .. ms_off + ms_len) */
  uint32_t ind_off, ind_len; /* Packet.IndividualSig = pool[ind_off .. ind_off + ind_len) */
} hg_packet;
#define HG_PKT_HAS_IND 1u
/* Words of bitset per request slot: ceil(largest level size / 64) for the
 * context's registry (the largest level holds 2^(ceil(log2 N) - 1) ids). */
size_t hg_packet_stride_words(hg_ctx* ctx);
/* Parses n packets against the context's registry size and flavor. Outputs
 * have 2n slots: slot i is packet i's multisignature, slot n + i its
 * individual signature as a one-bit multisignature of the level (handel.go:
 * 414-433). reqs[2n] (word_offset = slot * stride_words), words[2n *
 * stride_words] (bits at or above the bit length cleared), sigs[2n * 64] (the
 * signature marshal's first 64 bytes), codes[2n]: codes[i] = HG_OK or the
 * packet's first error in the reference's order; codes[n + i] = codes[i] if
 * that is an error, else HG_OK or HG_PKT_NO_IND. A packet whose individual
 * signature fails fails as a whole (parseSignatures returns the error and
 * NewPacket drops both). stride_words must be >= hg_packet_stride_words;
 * every pool range must lie inside pool_len (else HG_ERR_ARG). */
int hg_parse_packets(hg_ctx* ctx, const uint8_t* pool, size_t pool_len, const hg_packet* pkts, size_t n,
                     size_t stride_words, hg_request* reqs, uint64_t* words, uint8_t* sigs, int32_t* codes);
/* Device-resident variant (pool, pkts and every output on the device);
 * asynchronous on `stream`. A packet whose range leaves the pool gets
 * HG_ERR_ARG in its codes instead of a read outside it. */
int hg_parse_packets_device(hg_ctx* ctx, const uint8_t* d_pool, size_t pool_len, const hg_packet* d_pkts, size_t n,
                            size_t stride_words, hg_request* d_reqs, uint64_t* d_words, uint8_t* d_sigs,
                            int32_t* d_codes, void* stream);
/* The exact text the reference logs for packet p's code (with the level and
 * range values of the formatted errors), NUL-terminated into buf; returns the
 * full length (snprintf convention). */
int hg_packet_error(hg_ctx* ctx, int code, const hg_packet* p, char* buf, size_t cap);

/* ---------------------------------------------------------------- stores
 * The scoring step between parse and verify (processing.go:171-220 readTodos
 * over store.go:101-183 Evaluate), on the device. One hg_stores holds, for
 * every Handel instance (receiver) the process hosts and every level
 * 1..ceil(log2 N), the level's best bitset, whether there is one, and the
 * bitset of verified individual signatures (store.go:39-80), each
 * hg_packet_stride_words words, the two bitsets of a level adjacent. The host
 * store stays authoritative: Store / unsafeCheckMerge (store.go:82-226) run on
 * the host once per verified signature, and the levels that changed are pushed
 * with hg_stores_update; only the scoring of queued signatures runs here.
 * That is the default. A set that called hg_stores_enable_merge (the section
 * after this one) also holds the signatures and runs Store / unsafeCheckMerge
 * and Combined / FullSignature on the device; the host store is then a mirror
 * a caller may keep or drop.
 * A store set belongs to the registry its context held at hg_stores_create:
 * after a later hg_registry_load every call returns HG_ERR_ARG. Every call
 * is a submission of the context (ordered with parse and verify across
 * streams). Destroy the stores before their context. Registries of at most
 * 2^17 keys (a level's bit length is 16 bits on the wire). */
typedef struct hg_stores hg_stores;
typedef struct {
  uint32_t receiver; /* a hosted receiver id */
  uint32_t level;    /* one of the receiver's non-empty levels */
  uint32_t flags;    /* HG_STORE_HAS_BEST: the level has a best multisignature */
  uint32_t best_off, indiv_off; /* ceil(level size / 64) words each at words[off ...]; best_off unused without HAS_BEST */
} hg_store_update;
#define HG_STORE_HAS_BEST 1u
/* receivers: n_receivers >= 1 distinct ids below the registry size (else
 * HG_ERR_ARG); store index i = receivers[i]. max_packets >= 1 sizes the
 * workspaces of hg_stores_evaluate and hg_stores_select_device. Every level
 * starts without a best and without individual signatures. */
int hg_stores_create(hg_ctx* ctx, const uint32_t* receivers, size_t n_receivers, size_t max_packets, hg_stores** out);
void hg_stores_destroy(hg_stores* st);
/* Replaces the state of n (receiver, level) pairs, each named at most once:
 * one host-to-device copy and one scatter kernel. Bits at or above the
 * level's size are cleared on the way in. Synchronous (the inputs are free
 * on return). */
int hg_stores_update(hg_stores* st, const hg_store_update* ups, size_t n, const uint64_t* words, size_t nwords);
/* Reads one level back: best and indiv receive hg_packet_stride_words words
 * each (nullable), *has_best 0 or 1 (nullable). */
int hg_stores_read(hg_stores* st, uint32_t receiver, uint32_t level, uint64_t* best, uint64_t* indiv, int* has_best);
/* store.go:111-183 unsafeEvaluate for the 2n slots hg_parse_packets* wrote
 * (slot i: packet i's multisignature, slot n + i: its individual signature;
 * a slot's words at slot * stride_words; d_reqs is not needed: the level
 * range is recomputed from the packet's receiver and level). d_scores[slot]:
 *   0  when d_codes[slot] != HG_OK (HG_PKT_NO_IND included), when d_live
 *      (nullable, 2n bytes: the caller's IndividualSigFilter / rcvCompleted
 *      mask) holds 0 for the slot, or when the packet's (receiver, level) has
 *      no range, in this order; nothing else is read for such a slot;
 *   -1 when the receiver has no store (Handel's marks are never negative);
 *   else the reference's mark against the receiver's store at the packet's
 *   level: 0 for a completed level, a verified individual signature or a
 *   multisignature the best already covers, 1 for an individual signature
 *   that adds nothing, 1000000 - 10*level - combineCt when the level
 *   completes, else 100000 - 100*level + 10*addedSigs - combineCt.
 * stride_words >= hg_packet_stride_words. Asynchronous on `stream`. */
int hg_stores_evaluate_device(hg_stores* st, const hg_packet* d_pkts, size_t n, size_t stride_words,
                              const uint64_t* d_words, const int32_t* d_codes, const uint8_t* d_live,
                              int32_t* d_scores, void* stream);
/* The same with host pointers (n <= max_packets; words: 2n * stride_words). */
int hg_stores_evaluate(hg_stores* st, const hg_packet* pkts, size_t n, size_t stride_words, const uint64_t* words,
                       const int32_t* codes, const uint8_t* live, int32_t* scores);
/* Entries hg_stores_select_device writes: min(2n, n_receivers * k). */
size_t hg_stores_select_capacity(hg_stores* st, size_t n, uint32_t k);
/* readTodos with k slots per store (processing.go:171-220): per store the at
 * most k slots of score > 0 with the highest scores, among equal scores the
 * earliest in Handel's queue order, position 2*(slot mod n) + (slot >= n)
 * (a packet's multisignature before its individual signature, handel.go:
 * 145-149). Output grouped by store in creation order, inside a store by
 * score descending then position; the same input gives the same output.
 * d_sel[0 .. *d_count): the chosen slots; d_out_reqs / d_out_sigs: their
 * requests (word_offset untouched: they still point into the parsed words)
 * and 64-byte signatures, contiguous. Entries [*d_count, capacity) hold
 * 0xffffffff, a request that fails the level check (bitlen 0, level_size 1)
 * and a zero signature, so a caller may submit `capacity` requests to
 * hg_verify_aggregate_device without reading the count back. n <=
 * max_packets, k >= 1; d_sigs and d_out_sigs 4-byte aligned. Asynchronous on
 * `stream`. */
int hg_stores_select_device(hg_stores* st, const hg_packet* d_pkts, size_t n, const int32_t* d_scores, uint32_t k,
                            const hg_request* d_reqs, const uint8_t* d_sigs, uint32_t* d_sel, uint32_t* d_count,
                            hg_request* d_out_reqs, uint8_t* d_out_sigs, void* stream);

/* ---------------------------------------------------------------- stores: merge and Combined
 * Opt-in: the whole replace store on the device. After hg_stores_enable_merge
 * the set also holds, beside the bitsets above, the 64-byte marshal of every
 * level's best signature with a "best signature known" bit (HG_STORE_BEST_SIG
 * in the level's flags), the node's own signature as level 0 (handel.go:116:
 * one bit, one signature), every verified individual signature (store.go:58
 * individualSigs; one table of registry-size entries per store, entry = the
 * signer's registry id, the store's own id holding level 0) and a "signature
 * held" bitset per level. hg_stores_merge_device is then store.go:82-99 Store
 * (unsafeCheckMerge :188-229 + store :264-269) for the verified picks of an
 * intake step, and hg_stores_combined* store.go:238-262 FullSignature /
 * Combined (partitioner.go:224-296 Combine / CombineFull). A caller that runs
 * the merge here no longer runs Store / unsafeCheckMerge on the host; a set
 * that never calls hg_stores_enable_merge behaves and allocates as before, and
 * on it the entry points below (hg_stores_enable_merge apart) return
 * HG_ERR_ARG. Every signature that leaves the device is the marshal
 * SigBLS.MarshalBinary gives (bn256/go/bn256.go:170-172; infinity: 64 zero
 * bytes). Signatures are not checked here: they are verified ones, or the
 * caller's own. */
#define HG_STORE_BEST_SIG 2u /* level flags: the best's signature is held (cleared by hg_stores_update) */
#define HG_STORE_SIG_BEST 0xffffffffu   /* hg_store_sig.index: the level's best signature */
#define HG_STORE_LEVEL_FULL 0xffffffffu /* hg_store_query.level: FullSignature */
typedef struct {
  uint32_t receiver; /* a hosted receiver id */
  uint32_t level;    /* 0: the own signature (index ignored); else one of the receiver's non-empty levels */
  uint32_t index;    /* mapped index at the level (id - level min): an individual signature; HG_STORE_SIG_BEST */
  uint32_t sig_off;  /* the signature: sigs[64 * sig_off ...] */
} hg_store_sig;
typedef struct {
  uint32_t receiver; /* a hosted receiver id */
  uint32_t level;    /* 0 .. ceil(log2 N) - 1: Combined(level); HG_STORE_LEVEL_FULL */
} hg_store_query;
/* hg_stores_merge_device's result per entry */
enum {
  HG_MERGE_SKIPPED = 0,        /* verdict not HG_OK, or a filler entry */
  HG_MERGE_STORED = 1,         /* the level's best is now this entry's merge (store.go:95-97) */
  HG_MERGE_DISCARDED = 2,      /* unsafeCheckMerge returned false (store.go:211-213) */
  HG_MERGE_ERR_MISSING = 3,    /* a needed best or individual signature is not held (store.go:219 panics) */
  HG_MERGE_ERR_INDIVIDUAL = 4, /* an individual slot whose bitset is not its one bit (store.go:87-89 panics) */
  HG_MERGE_ERR_ROW = 5         /* the slot's packet names no (store, level) of this set */
};
/* hg_stores_combined*'s code per query (HG_OK, HG_ERR_ARG: the level is neither
 * below ceil(log2 N) nor HG_STORE_LEVEL_FULL, the receiver is not hosted, or
 * the bitset does not fit words_stride) */
#define HG_COMBINED_EMPTY 1       /* no best at those levels: the reference returns nil (partitioner.go:225-227) */
#define HG_COMBINED_ERR_MISSING 2 /* a level has a best whose signature is not held */
/* Allocates the signature tables (idempotent). Levels that already have a best
 * (hg_stores_update) keep it without a signature until hg_stores_update_sigs
 * gives one. */
int hg_stores_enable_merge(hg_stores* st);
/* Loads n signatures from the host (seeding, and a host store's mirror), each
 * target named at most once: an individual signature (sets its "held" bit, not
 * the verified bit: that is hg_stores_update's bitset), a level's best
 * signature (sets HG_STORE_BEST_SIG), or the own signature (level 0; it is the
 * level-0 best, crypto.go / handel.go:116). sigs holds n_sigs 64-byte
 * marshals. Synchronous. */
int hg_stores_update_sigs(hg_stores* st, const hg_store_sig* recs, size_t n, const uint8_t* sigs, size_t n_sigs);
/* Reads one level back (store.go:231-236 Best): best receives
 * hg_packet_stride_words words, sig the best's 64-byte marshal, *flags
 * HG_STORE_HAS_BEST | HG_STORE_BEST_SIG as they hold (each nullable). Level 0:
 * word 0 bit 0 and both flags say whether the own signature is held. */
int hg_stores_read_best(hg_stores* st, uint32_t receiver, uint32_t level, uint64_t* best, uint8_t* sig, int* flags);
/* store.go:82-99 Store for the picks of one intake step. d_sel[e] names the
 * slot of entry e (hg_stores_select_device's output; >= 2n: a filler),
 * d_vcodes[e] its verdict (hg_verify_aggregate_device); entries e <
 * min(*d_count, capacity), or all `capacity` with d_count NULL. d_pkts[n],
 * d_words (slot * stride_words) and d_sigs (slot * 64) are the parse outputs.
 * The entries whose verdict is HG_OK are applied to their (receiver, level) in
 * array order; every level ends in the state the reference's store reaches
 * when fed those entries in that order: an individual slot (>= n) first sets
 * its verified bit and keeps its signature (store.go:86-92); then
 * unsafeCheckMerge: without a best the entry becomes the best; else the
 * candidate is the union with the best and the G1 sum of both signatures
 * (bn256/go/bn256.go:192-200 Combine) when the two sets are disjoint, the
 * entry itself otherwise; with iS the verified individual signatures outside
 * the candidate, the entry is discarded when |iS| + |candidate| <= |best|,
 * else every signature of iS joins the candidate, which becomes the best.
 * An entry that ends in an error changes nothing. d_results[capacity]: HG_MERGE_*
 * (entries past the count: HG_MERGE_SKIPPED). d_changed[2 * capacity]:
 * (receiver, level) of the levels whose best changed, ordered by their first
 * entry, *d_nchanged of them. n <= max_packets, capacity <= 2 * max_packets,
 * stride_words >= hg_packet_stride_words, d_sigs 4-byte aligned. Asynchronous
 * on `stream`. */
int hg_stores_merge_device(hg_stores* st, const hg_packet* d_pkts, size_t n, const uint32_t* d_sel,
                           const uint32_t* d_count, size_t capacity, const int32_t* d_vcodes, size_t stride_words,
                           const uint64_t* d_words, const uint8_t* d_sigs, int32_t* d_results, uint32_t* d_changed,
                           uint32_t* d_nchanged, void* stream);
/* store.go:248-262 Combined(level) / :238-246 FullSignature for m queries, all
 * pointers on the device. Combined(level): the bests of levels <= level, level
 * 0 included, each at rangeLevel(k).min - rangeLevelInverse(level + 1).min in
 * a bitset of rangeLevelInverse(level + 1)'s size (partitioner.go:185-211,
 * 224-261), their signatures summed; HG_STORE_LEVEL_FULL: every level at its
 * rangeLevel min in a registry-size bitset (:263-278). Per query q:
 * d_codes[q], d_bitlens[q], d_words[q * words_stride ...] (words_stride words,
 * zero above the bit length) and d_sigs[64 * q ...]; a query whose code is not
 * HG_OK leaves zero words and a zero signature. Asynchronous on `stream`. */
int hg_stores_combined_device(hg_stores* st, const hg_store_query* d_queries, size_t m, size_t words_stride,
                              int32_t* d_codes, uint32_t* d_bitlens, uint64_t* d_words, uint8_t* d_sigs,
                              void* stream);
/* The same with host pointers. Synchronous. */
int hg_stores_combined(hg_stores* st, const hg_store_query* queries, size_t m, size_t words_stride, int32_t* codes,
                       uint32_t* bitlens, uint64_t* words, uint8_t* sigs);

/* ---------------------------------------------------------------- stores: the standing queue
 * Opt-in: Handel's queue of parsed signatures in HBM. readTodos
 * (processing.go:171-220) verifies the best signatures of a pass and keeps
 * every other one of positive mark for the next. A pool holds those slots on
 * the device between intake steps: hg_stores_pool_append_device adds the
 * admitted slots of a parsed batch, hg_stores_pool_step_device scores every
 * pooled slot against the stores as they are now, hands out the k best per
 * store as a parsed batch (for hg_verify_aggregate_device and
 * hg_stores_merge_device) and re-queues the rest in readTodos' order. A pooled
 * slot holds its packet's origin, receiver, level and flags, whether it is the
 * individual slot, its request's offset, bitlen and level_size (32 bytes),
 * hg_packet_stride_words bitset words, the 64-byte signature and its last
 * mark; its place in its receiver's queue is its index (among one receiver's
 * slots a lower index is earlier). The pool keeps two such sides, a step
 * writing the survivors from one to the other.
 * A pool belongs to one hg_stores and through it to one context and registry:
 * after a later hg_registry_load every call returns HG_ERR_ARG. Every call is
 * a submission of the context. Destroy the pool before its stores. */
typedef struct hg_pool hg_pool;
/* capacity_slots >= 1 (at most 2^25). Everything the pool needs, workspaces
 * included, is allocated here; no later call allocates device memory. */
int hg_stores_pool_create(hg_stores* st, size_t capacity_slots, hg_pool** out);
void hg_stores_pool_destroy(hg_pool* pool);
/* Device memory the pool holds, in bytes. */
size_t hg_stores_pool_bytes(hg_pool* pool);
/* Appends the slots of one hg_parse_packets_device call (its inputs d_pkts, n,
 * stride_words and its outputs). A slot is admitted if and only if its code is
 * HG_OK, its d_live byte (nullable, 2n bytes) is not 0, its (receiver, level)
 * has a range and its receiver has a store: the slots hg_stores_evaluate_device
 * scores against a store. Admitted slots are queued in Handel's queue order,
 * 2*(slot mod n) + (slot >= n), each behind everything its receiver already
 * has queued. Asynchronous on `stream`. The pool keeps a host-side bound on
 * its occupancy: the last count it read back plus every slot offered since.
 * When the bound plus 2n exceeds the capacity the call reads the true count
 * (one synchronisation of the stream); when 2n still does not fit it returns
 * HG_ERR_ARG and appends nothing. Whatever the host believes, no kernel writes
 * at an index at or above the capacity. d_sigs 4-byte aligned. */
int hg_stores_pool_append_device(hg_pool* pool, const hg_packet* d_pkts, size_t n, size_t stride_words,
                                 const hg_request* d_reqs, const uint64_t* d_words, const uint8_t* d_sigs,
                                 const int32_t* d_codes, const uint8_t* d_live, void* stream);
/* Entries hg_stores_pool_step_device writes: min(capacity_slots, n_receivers * k). */
size_t hg_stores_pool_select_capacity(hg_pool* pool, uint32_t k);
/* One pass of readTodos with k slots per store (1 <= k <= 64) over the whole
 * pool. Every pooled slot gets store.go:111-183 unsafeEvaluate's mark against
 * the stores as they are now. Per store at most k slots of mark > 0 are
 * picked, highest mark first, equal marks by earlier queue place; the output
 * is grouped by store in creation order (hg_stores_select_device's rule and
 * order). The picks and every slot of mark <= 0 leave the pool; the others
 * stay, per store in the order readTodos re-queues them (a slot that loses on
 * arrival is appended when it is met, one pushed out of the k held when it is
 * pushed out). The output is a parsed batch of `capacity` packets, capacity =
 * hg_stores_pool_select_capacity(pool, k) <= the store set's max_packets
 * (else HG_ERR_ARG): entry e < *d_count has its packet record (pool offsets
 * zero) in d_out_pkts[e]; its slot d_sel[e] is e for a multisignature and
 * capacity + e for an individual signature; d_out_reqs[e].word_offset =
 * d_sel[e] * hg_packet_stride_words, its words at that slot of d_out_words
 * (2 * capacity slots), its signature at 64 * e and, for an individual slot,
 * also at 64 * (capacity + e) of d_out_sigs (2 * capacity * 64 bytes, 4-byte
 * aligned); d_out_scores[e] is its mark. Entries from *d_count on are
 * hg_stores_select_device's filler: slot 0xffffffff, request {0, 0, 1, 0}, a
 * zero signature, a zero record and mark. So
 * hg_verify_aggregate_device(d_out_reqs, capacity, d_out_words, d_out_sigs, ..)
 * and hg_stores_merge_device(st, d_out_pkts, capacity, d_sel, d_count,
 * capacity, d_vcodes, stride, d_out_words, d_out_sigs, ..) run on the output
 * as it is. Slots of d_out_words and d_out_sigs that no entry names are not
 * written. Asynchronous on `stream`; the same pool state and stores give the
 * same output. */
int hg_stores_pool_step_device(hg_pool* pool, uint32_t k, size_t capacity, hg_packet* d_out_pkts, uint32_t* d_sel,
                               uint32_t* d_count, hg_request* d_out_reqs, uint64_t* d_out_words, uint8_t* d_out_sigs,
                               int32_t* d_out_scores, void* stream);
/* Slots queued now. Synchronous; refreshes the host-side bound. */
int hg_stores_pool_count(hg_pool* pool, size_t* count);
/* Read-back for tests and diagnosis: the queued slots of one hosted receiver
 * in queue order, the first `cap` of them: packet record, whether it is the
 * individual slot, and the mark it got in the last step (0 for a slot
 * appended since); each array nullable. *count: how many the receiver has
 * queued. Synchronous. */
int hg_stores_pool_read(hg_pool* pool, uint32_t receiver, size_t cap, hg_packet* pkts, uint8_t* individual,
                        int32_t* scores, size_t* count);
/* Empties the pool. Synchronous. */
int hg_stores_pool_clear(hg_pool* pool);

/* ---------------------------------------------------------------- batcher
 * A launch-merging request queue on one context, for callers that verify one
 * multisignature at a time: each Handel instance's processLoop checks one
 * signature per step (processing.go:228-287 -> verifySignature :342-368) and
 * a simul process runs k instances concurrently (simul/node/main.go:63-131).
 * A dispatcher thread merges the queued requests into one
 * hg_verify_aggregate_msg batch (grouped by message, at most max_batch; an
 * idle dispatcher waits at most max_wait_us after the oldest request for
 * more) and hands every caller its own code. Verdicts are a pure function of
 * (msg, range, bitset, sig), so batching cannot change them. The context must
 * outlive the batcher. */
typedef struct hg_batcher hg_batcher;
typedef struct hg_ticket hg_ticket;
int hg_batcher_create(hg_ctx* ctx, size_t max_batch, unsigned max_wait_us, hg_batcher** out);
/* Verifies what is still queued, then stops the dispatcher. Tickets stay
 * valid: hg_batcher_wait on a ticket submitted before the destroy returns its
 * code even after the batcher is gone (a ticket holds its own state). */
void hg_batcher_destroy(hg_batcher* b);
/* Queues one request: req->offset / bitlen / level_size as in hg_request
 * (word_offset ignored), its ceil(bitlen/64) bitset words at `words`, the
 * 64-byte signature. Inputs are copied; the ticket is released by
 * hg_batcher_wait, exactly once. */
int hg_batcher_submit(hg_batcher* b, const uint8_t* msg, size_t len, const hg_request* req, const uint64_t* words,
                      const uint8_t* sig, hg_ticket** out);
/* Blocks until the ticket's batch ran; *code = its hg_code. Returns HG_OK, or
 * the batch's HG_ERR_ARG / HG_ERR_DEVICE. */
int hg_batcher_wait(hg_batcher* b, hg_ticket* t, int32_t* code);
/* hg_batcher_submit + hg_batcher_wait: one processing.go verifySignature. */
int hg_batcher_verify_aggregate(hg_batcher* b, const uint8_t* msg, size_t len, const hg_request* req,
                                const uint64_t* words, const uint8_t* sig, int32_t* code);
int hg_batcher_stats(hg_batcher* b, uint64_t* batches, uint64_t* requests);

/* ---------------------------------------------------------------- lanes
 * Several aggregate batches of one context in flight at once. A lane owns a
 * stream, device workspaces and pinned host staging; lanes share the
 * context's registry, hashed message and GT tables, which are read-only while
 * lanes run. A lane batch verifies against the context's CURRENT message
 * (hg_set_message / hg_prepare_aggregate_msg, called with every lane idle)
 * at the table level already built (hg_prepare_aggregate*): a lane never
 * builds tables. Used by the verifier service below; one thread per lane.
 * Lanes must be destroyed before their context. */
typedef struct hg_lane hg_lane;
/* max_batch requests and max_words bitset words per batch; overlap: the GT
 * fold beside the pairing kernel on a second stream of the lane. */
int hg_lane_create(hg_ctx* ctx, size_t max_batch, size_t max_words, int overlap, hg_lane** out);
void hg_lane_destroy(hg_lane* lane);
/* Pinned staging of the next batch: n requests (word_offset relative to
 * *words), their 64-byte signatures, nwords bitset words. The lane must be
 * idle. The pointers stay valid until the next hg_lane_stage. */
int hg_lane_stage(hg_lane* lane, size_t n, size_t nwords, hg_request** reqs, uint8_t** sigs, uint64_t** words);
/* Enqueues the staged batch (one host-to-device copy, the GT or G2 path,
 * the codes back to pinned memory); asynchronous. */
int hg_lane_submit(hg_lane* lane);
/* 1: the last batch is done (hg_lane_codes valid), 0: running, else an error code. */
int hg_lane_query(hg_lane* lane);
int hg_lane_wait(hg_lane* lane);
/* The last batch's n codes (pinned host memory, valid once it is done). */
const int32_t* hg_lane_codes(hg_lane* lane);
/* A batch already in HBM through the lane (the device twin of
 * hg_verify_aggregate_device_bits): enqueued on the lane's streams after the
 * caller's earlier work on `stream` (NULL: the context's stream), and `stream`
 * waits for the verdicts, so the caller reads d_codes / d_bits in its own
 * stream order while the next batch runs on another lane. d_bits may be NULL.
 * hg_lane_codes does not apply; hg_lane_query / hg_lane_wait do. */
int hg_lane_submit_device(hg_lane* lane, const hg_request* d_reqs, size_t n, const uint64_t* d_words,
                          const uint8_t* d_sigs, int32_t* d_codes, uint8_t* d_bits, void* stream);
/* 1 (the default): the lane's pairing kernel holds one wave per SIMD (the
 * lowest latency for one batch); 0: unpadded, so two batches in flight put
 * two pairing waves on a SIMD (throughput of a continuous stream). */
int hg_lane_set_pairing_padding(hg_lane* lane, int pad);
/* The latency form on a padded lane: its batches of at most max_checks
 * (<= 2048) checks run the pairing with each check's team over two waves
 * (k_verify_sig_split<2>: ~9 % shorter, twice the waves); 0 (the default,
 * or HG_SIG_W2_LANE_MAX): never. The verifier service sets it per batch while
 * the batches in flight leave a SIMD per wave. Takes effect at the next
 * submission. */
int hg_lane_set_latency_form(hg_lane* lane, int max_checks);
/* The lane's launch stream (a hipStream_t): passed as hg_lane_submit_device's
 * `stream`, the lane orders its batches only after its own earlier ones. */
void* hg_lane_stream(hg_lane* lane);
/* Builds the GT tables of the current message up to `level` (0..2, capped as
 * hg_prepare_aggregate caps) now; for owners of lanes that follow the volume
 * policy themselves. Synchronous. */
int hg_prepare_aggregate_level(hg_ctx* ctx, int level);

/* ---------------------------------------------------------------- verifier service
 * ONE process owns the GPU, the context, the registry and ONE set of GT
 * tables, and verifies the aggregate checks of many client processes that
 * reach it through a POSIX shared-memory object `name` (shm_open). Clients
 * use include/handel_client.h (libhandel_client.so: no GPU, no HIP runtime),
 * so simul's single-host layout — P OS processes of k Handel instances each
 * (simul/node/main.go:63-131), every instance's evaluator checking one
 * multisignature at a time (processing.go:228-287 -> verifySignature
 * :342-368) — shares one GPU without a HIP context per process. A dispatcher
 * thread merges queued requests into batches (grouped by message, at most
 * max_batch) and keeps up to `lanes` batches in flight (hg_lane_*); each
 * client learns its own verdicts. The context must outlive the service and
 * must not be used by others while it runs (the service switches its message
 * and builds its tables). */
typedef struct hg_service hg_service;
typedef struct {
  uint32_t slots;       /* request slots in the region (multiple of 64; default 8192) */
  uint32_t slot_bits;   /* largest bitset of one request (default: the registry size) */
  uint32_t channels;    /* client handles attached at once (default 256) */
  uint32_t lanes;       /* batches in flight on the GPU (default 8) */
  uint32_t max_batch;   /* requests per batch (default 4096) */
  uint32_t max_wait_us; /* a queued request waits at most this long for more to batch with (default 50) */
  uint32_t quiet_us;    /* ... or until no request has arrived for quiet_us (0 = off; the default) */
  int32_t prepare;      /* 1 (default): a message's first batch builds its top GT table level;
                           0: the context's volume policy (levels 1 and 2 after 16384 / 2^20 requests) */
  int32_t overlap;      /* 1 (default): the GT fold beside the pairing kernel inside each lane */
  int32_t follow;       /* 1 (default): ... or as soon as as many requests have arrived as finished
                           batches released (clients that submit their next check on a verdict:
                           the whole cohort is back), whichever comes first; 0: off */
} hg_service_config;
void hg_service_config_init(hg_service_config* cfg);
/* Creates the region (fails if `name` exists) and starts the dispatcher. */
int hg_service_create(hg_ctx* ctx, const char* name, const hg_service_config* cfg, hg_service** out);
/* The same protocol served by a CPU stand-in for the GPU (protocol tests
 * without a GPU): a request's code is HG_ERR_LEVEL if it fails the level
 * check against an nreg-key registry, 77 if its bitset words do not match
 * sig[1..8] (the xor of the words, little-endian), else HG_ERR_SIG_INVALID
 * if sig[0] == 1, else HG_OK; each batch completes delay_us after launch. */
int hg_service_create_echo(const char* name, const hg_service_config* cfg, uint32_t nreg, uint32_t delay_us,
                           hg_service** out);
/* Verifies what is queued, stops the dispatcher, wakes every client and
 * removes the region's name. */
void hg_service_destroy(hg_service* svc);
/* batches launched, requests verified, most batches in flight at once */
int hg_service_stats(hg_service* svc, uint64_t* batches, uint64_t* requests, uint64_t* max_in_flight);

#ifdef __cplusplus
}
#endif
#endif /* HANDEL_GPU_H */
