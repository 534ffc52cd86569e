// bn256_fprobe.hip — hg_debug_field's kernels: ONE per-thread primitive of
// bn256_fp.h / bn256_curve.h per launch, one thread per case, on raw limbs,
// for the bit-exact comparison with Python integers
// (tests/test_field_edges.py, tests/test_gpu_field.py).
//
// An Fp element travels as its ten 32-bit words Fp::l, an Fp2 as x then y, a
// Jacobian point as x, y, z: no Montgomery conversion and no reduction on the
// way in or out, so the test chooses the limb patterns. Every op calls the
// production function itself. One kernel per op (the op is a template
// parameter): the G2 bodies take about a SIMD's VGPRs, which a switch in one
// kernel would impose on the Fp ops too.
#include <hip/hip_runtime.h>

#include "bn256_curve.h"
#include "bn256_kernels.h"

namespace hg {

// X(number, name, words in, words out); the numbers are the ABI (include/handel_gpu.h)
#define HG_FPROBE_OPS(X)          \
  X(0, FP_ADD, 20, 10)            \
  X(1, FP_SUB, 20, 10)            \
  X(2, FP_NEG, 10, 10)            \
  X(3, FP_DBL, 10, 10)            \
  X(4, FP_MUL3, 10, 10)           \
  X(5, FP_MUL, 20, 10)            \
  X(6, FP_SQR, 10, 10)            \
  X(7, FP_INV, 10, 10)            \
  X(8, FP_NEG_LOOSE, 10, 10)      \
  X(9, FP_ADD_LOOSE, 20, 10)      \
  X(10, FP_TO_MONT, 8, 10)        \
  X(11, FP_FROM_MONT, 10, 8)      \
  X(12, FP_FROM_BE, 10, 12)       \
  X(13, FP_TO_BE, 10, 8)          \
  X(14, F2_MUL, 40, 20)           \
  X(15, F2_SQR, 20, 20)           \
  X(16, F2_MULS, 30, 20)          \
  X(17, F2_MUL_XI, 20, 20)        \
  X(18, F2_INV, 20, 20)           \
  X(19, F2_SUB, 40, 20)           \
  X(20, F2_NEG, 20, 20)           \
  X(21, F2_CONJ, 20, 20)          \
  X(22, G1_DOUBLE, 30, 30)        \
  X(23, G1_ADD, 60, 30)           \
  X(24, G1_MADD, 50, 30)          \
  X(25, G1_ON_CURVE, 20, 1)       \
  X(26, G1_AFFINE, 30, 20)        \
  X(27, G2_DOUBLE, 60, 60)        \
  X(28, G2_ADD, 120, 60)          \
  X(29, G2_MADD, 100, 60)         \
  X(30, G2_ADD_AFFINE, 100, 60)   \
  X(31, G2_ON_CURVE, 40, 1)       \
  X(32, G2_AFFINE, 60, 40)

enum FProbeOp : int {
#define HG_FPROBE_ENUM(N, NAME, IN, OUT) FPO_##NAME = N,
  HG_FPROBE_OPS(HG_FPROBE_ENUM)
#undef HG_FPROBE_ENUM
  kFProbeOps
};

struct FProbeWords {
  int in, out;
};
static constexpr FProbeWords kFProbeWords[kFProbeOps] = {
#define HG_FPROBE_WORDS(N, NAME, IN, OUT) {IN, OUT},
    HG_FPROBE_OPS(HG_FPROBE_WORDS)
#undef HG_FPROBE_WORDS
};

// operand k of a case: ten words, as Fp::l
HG_DEV void fpr_ld(Fp& r, const uint32_t* w, int k) {
#pragma unroll
  for (int i = 0; i < 10; i++) r.l[i] = w[10 * k + i];
}
HG_DEV void fpr_ld2(Fp2& r, const uint32_t* w, int k) {
  fpr_ld(r.x, w, k);
  fpr_ld(r.y, w, k + 1);
}
HG_DEV void fpr_st(uint32_t* w, int k, const Fp& a) {
#pragma unroll
  for (int i = 0; i < 10; i++) w[10 * k + i] = a.l[i];
}
HG_DEV void fpr_st2(uint32_t* w, int k, const Fp2& a) {
  fpr_st(w, k, a.x);
  fpr_st(w, k + 1, a.y);
}
HG_DEV void fpr_ldj(G1J& r, const uint32_t* w, int k) {
  fpr_ld(r.x, w, k);
  fpr_ld(r.y, w, k + 1);
  fpr_ld(r.z, w, k + 2);
}
HG_DEV void fpr_ldj(G2J& r, const uint32_t* w, int k) {
  fpr_ld2(r.x, w, k);
  fpr_ld2(r.y, w, k + 2);
  fpr_ld2(r.z, w, k + 4);
}
HG_DEV void fpr_stj(uint32_t* w, const G1J& a) {
  fpr_st(w, 0, a.x);
  fpr_st(w, 1, a.y);
  fpr_st(w, 2, a.z);
}
HG_DEV void fpr_stj(uint32_t* w, const G2J& a) {
  fpr_st2(w, 0, a.x);
  fpr_st2(w, 2, a.y);
  fpr_st2(w, 4, a.z);
}

// in, out: n cases of kFProbeWords[OP].in / .out words
template <int OP>
__global__ __launch_bounds__(64) void k_fprobe(const uint32_t* in, int n, uint32_t* out) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= n) return;
  const uint32_t* a = in + (size_t)idx * kFProbeWords[OP].in;
  uint32_t* o = out + (size_t)idx * kFProbeWords[OP].out;
  if constexpr (OP <= FPO_FP_ADD_LOOSE) {
    Fp x, y, r;
    fpr_ld(x, a, 0);
    if constexpr (kFProbeWords[OP].in == 20) fpr_ld(y, a, 1);
    if constexpr (OP == FPO_FP_ADD) fp_add(r, x, y);
    else if constexpr (OP == FPO_FP_SUB) fp_sub(r, x, y);
    else if constexpr (OP == FPO_FP_NEG) fp_neg(r, x);
    else if constexpr (OP == FPO_FP_DBL) fp_dbl(r, x);
    else if constexpr (OP == FPO_FP_MUL3) fp_mul3(r, x);
    else if constexpr (OP == FPO_FP_MUL) fp_mul(r, x, y);
    else if constexpr (OP == FPO_FP_SQR) fp_sqr(r, x);
    else if constexpr (OP == FPO_FP_INV) fp_inv(r, x);
    else if constexpr (OP == FPO_FP_NEG_LOOSE) fp_neg_loose(r, x);
    else fp_add_loose(r, x, y);
    fpr_st(o, 0, r);
  } else if constexpr (OP == FPO_FP_TO_MONT) {
    Fp x, r;
    words_to_limbs(x, a);
    fp_to_mont(r, x);
    fpr_st(o, 0, r);
  } else if constexpr (OP == FPO_FP_FROM_MONT) {
    Fp x, r;
    fpr_ld(x, a, 0);
    fp_from_mont(r, x);
    uint32_t w[8];
    limbs_to_words(w, r);
#pragma unroll
    for (int i = 0; i < 8; i++) o[i] = w[i];
  } else if constexpr (OP == FPO_FP_FROM_BE) {
    // word 0: the byte offset k in 0..3; words 1..9: a 36-byte buffer with the
    // 32 bytes at its byte k (k = 0: be_to_words' dword path, else its byte path)
    const uint8_t* b = reinterpret_cast<const uint8_t*>(a + 1) + (a[0] & 3);
    Fp r;
    bool ge = false, nz = false;
    fp_from_be(r, b, &ge, &nz);
    fpr_st(o, 0, r);
    o[10] = ge ? 1 : 0;
    o[11] = nz ? 1 : 0;
  } else if constexpr (OP == FPO_FP_TO_BE) {
    Fp x;
    fpr_ld(x, a, 0);
    fp_to_be(reinterpret_cast<uint8_t*>(o), x);
  } else if constexpr (OP <= FPO_F2_CONJ) {
    Fp2 x, y, r;
    fpr_ld2(x, a, 0);
    if constexpr (OP == FPO_F2_MUL) {
      fpr_ld2(y, a, 2);
      f2_mul(r, x, y);
    } else if constexpr (OP == FPO_F2_SQR) {
      f2_sqr(r, x);
    } else if constexpr (OP == FPO_F2_MULS) {
      Fp s;
      fpr_ld(s, a, 2);
      f2_muls(r, x, s);
    } else if constexpr (OP == FPO_F2_MUL_XI) {
      f2_mul_xi(r, x);
    } else if constexpr (OP == FPO_F2_INV) {
      f2_inv(r, x);
    } else if constexpr (OP == FPO_F2_SUB) {
      fpr_ld2(y, a, 2);
      f2_sub(r, x, y);
    } else if constexpr (OP == FPO_F2_NEG) {
      f2_neg(r, x);
    } else {
      f2_conj(r, x);
    }
    fpr_st2(o, 0, r);
  } else if constexpr (OP == FPO_G1_DOUBLE || OP == FPO_G1_ADD || OP == FPO_G1_MADD) {
    G1J p, r;
    fpr_ldj(p, a, 0);
    if constexpr (OP == FPO_G1_DOUBLE) {
      g1_double(r, p);
    } else if constexpr (OP == FPO_G1_ADD) {
      G1J q;
      fpr_ldj(q, a, 3);
      g1_add(r, p, q);
    } else {
      Fp bx, by;
      fpr_ld(bx, a, 3);
      fpr_ld(by, a, 4);
      g1_madd(r, p, bx, by);
    }
    fpr_stj(o, r);
  } else if constexpr (OP == FPO_G1_ON_CURVE) {
    Fp x, y;
    fpr_ld(x, a, 0);
    fpr_ld(y, a, 1);
    o[0] = g1_on_curve(x, y) ? 1 : 0;
  } else if constexpr (OP == FPO_G1_AFFINE) {
    G1J p;
    fpr_ldj(p, a, 0);
    Fp x, y;
    g1_affine(x, y, p);
    fpr_st(o, 0, x);
    fpr_st(o, 1, y);
  } else if constexpr (OP == FPO_G2_ON_CURVE) {
    Fp2 x, y;
    fpr_ld2(x, a, 0);
    fpr_ld2(y, a, 2);
    o[0] = g2_on_curve(x, y) ? 1 : 0;
  } else if constexpr (OP == FPO_G2_AFFINE) {
    G2J p;
    fpr_ldj(p, a, 0);
    Fp2 x, y;
    g2_affine(x, y, p);
    fpr_st2(o, 0, x);
    fpr_st2(o, 2, y);
  } else {
    G2J p, r;
    fpr_ldj(p, a, 0);
    if constexpr (OP == FPO_G2_DOUBLE) {
      g2_double(r, p);
    } else if constexpr (OP == FPO_G2_ADD) {
      G2J q;
      fpr_ldj(q, a, 6);
      g2_add(r, p, q);
    } else {
      Fp2 bx, by;
      fpr_ld2(bx, a, 6);
      fpr_ld2(by, a, 8);
      if constexpr (OP == FPO_G2_MADD) g2_madd(r, p, bx, by);
      else g2_add_affine(r, p, bx, by);
    }
    fpr_stj(o, r);
  }
}

// the words of one case of op going in and coming out; false: no such op
bool fprobe_words(int op, int* in_words, int* out_words) {
  if (op < 0 || op >= kFProbeOps) return false;
  *in_words = kFProbeWords[op].in;
  *out_words = kFProbeWords[op].out;
  return true;
}

// the caller has checked op with fprobe_words
void launch_fprobe(int op, const uint32_t* in, int n, uint32_t* out, hipStream_t s) {
  if (n <= 0) return;
  switch (op) {
#define HG_FPROBE_CASE(N, NAME, IN, OUT) \
  case N: k_fprobe<N><<<(n + 63) / 64, 64, 0, s>>>(in, n, out); break;
    HG_FPROBE_OPS(HG_FPROBE_CASE)
#undef HG_FPROBE_CASE
    default: break;
  }
}

}  // namespace hg
