// TEST-ONLY host build of the device arithmetic headers (bigfield.hpp / ec.hpp / smallfield.hpp)
// with the debug bound tracker on (-DBIGFIELD_BOUNDS). Lets the CPU test-suite check the exact
// code the kernels run against Python big-int arithmetic and the reference oracle, without a GPU.
// Not part of the shipped library; nothing in icicle_amd/ links it.
#include <cstdint>
#include <cstring>
#include "math_cases.hpp"
#include "../icicle_amd/csrc/glv.hpp"
#include "../icicle_amd/csrc/ec_dbl_quad.hpp"

using namespace icicle_hip;

namespace {
  // the case bodies shared with the device harness live in math_cases.hpp
  template <class PR>
  int field_op(int op, const uint32_t* a, const uint32_t* b, uint32_t* out)
  {
    if (op < 0 || op > 9) return -1;
    return math_cases::field_case<FieldOps<PR>>(op, a, b, a, b, out);
  }

  // points: affine canonical words (x,y); identity (0,0)
  template <class C>
  int ec_op(int op, const uint32_t* pts, int n, const uint32_t* aux, uint32_t* out)
  {
    using E = EC<C>;
    using F = typename E::F;
    constexpr int N32 = E::N32;
    auto load = [&](const uint32_t* w) {
      typename E::Aff a;
      a.x = F::from_canonical(w);
      a.y = F::from_canonical(w + N32);
      return a;
    };
    switch (op) {
    case 0:
    case 1:
    case 2:
    case 3:
    case 4:
    case 5:
    case 6: return math_cases::ec_case<C>(op, pts, n, aux, out);
    case 7: { // the ECNTT's scalar multiplication (ecntt.hip mul_words_quad, one lane's arithmetic): aux[0..7] * pts[0] by the GLV split, 27 joint
              // signed five-bit windows over the multiples 1..16, five complete projective doublings per window (ec_dbl_quad.hpp) and complete additions
      if constexpr (has_small_b3<C>::value) {
        using Proj = typename E::Proj;
        const Proj p = E::words_are_zero(pts) ? E::proj_identity() : E::to_proj(load(pts));
        Proj tab[16];
        uint32_t k1[5], k2[5];
        bool n1, n2;
        glv_decompose<C>(aux, k1, n1, k2, n2);
        const typename F::fe beta = F::from_const(C::GLV_BETA);
        Proj r = E::proj_identity();
        bool started = false;
        Proj e = p;
        for (int i = 0; i < 16; i++) {
          tab[i] = e;
          if (i < 15) e = (i == 0) ? EcDblSmallB<C>::dbl(p) : E::add(e, p);
        }
        uint32_t pk1[7], pk2[7];
        glv_recode5(k1, pk1);
        glv_recode5(k2, pk2);
        for (int d = 26; d >= 0; d--) {
          const uint32_t b1 = (pk1[d >> 2] >> ((d & 3) * 8)) & 0xFFu, b2 = (pk2[d >> 2] >> ((d & 3) * 8)) & 0xFFu;
          if (started)
            for (int q = 0; q < 5; q++)
              r = EcDblSmallB<C>::dbl(r); // the quad form's operand flow on one lane
          if (b1 & 31u) {
            Proj t = tab[(b1 & 31u) - 1];
            if (n1 != ((b1 & 0x80u) != 0)) t.y = F::template neg<4>(F::below4(t.y));
            r = started ? E::add(r, t) : t;
            started = true;
          }
          if (b2 & 31u) {
            Proj t = tab[(b2 & 31u) - 1];
            t.x = F::mul(t.x, beta);
            if (n2 != ((b2 & 0x80u) != 0)) t.y = F::template neg<4>(F::below4(t.y));
            r = started ? E::add(r, t) : t;
            started = true;
          }
        }
        // (the butterfly then forms u + v and u - v: the negation of the result must be in bounds as well)
        Proj nr = r;
        nr.y = F::template neg<4>(r.y);
        E::store_proj_canonical(out, E::add(E::add(r, nr), r));
        return 0;
      }
      return -1;
    }
    default: return -1;
    }
  }
} // namespace

// GLV decomposition (glv.hpp): out = |k1| (5 words), neg1, |k2| (5 words), neg2
extern "C" int host_glv_decompose(int curve, const uint32_t* k, uint32_t* out)
{
  bool n1 = false, n2 = false;
  switch (curve) {
  case 0: glv_decompose<bn254_g1>(k, out, n1, out + 6, n2); break;
  case 1: glv_decompose<bls12_381_g1>(k, out, n1, out + 6, n2); break;
  case 4: glv_decompose<bls12_377_g1>(k, out, n1, out + 6, n2); break;
  case 5: glv_decompose<grumpkin_g1>(k, out, n1, out + 6, n2); break;
  default: return -1;
  }
  out[5] = n1, out[11] = n2;
  return 0;
}

// signed five-bit recoding (glv.hpp glv_recode5): k (5 words) -> 27 digits as int32
extern "C" int host_glv_recode5(const uint32_t* k, int32_t* digits)
{
  uint32_t pk[7];
  glv_recode5(k, pk);
  for (int i = 0; i < 27; i++) {
    const uint32_t b = (pk[i >> 2] >> ((i & 3) * 8)) & 0xFFu;
    digits[i] = (b & 0x80u) ? -(int32_t)(b & 31u) : (int32_t)(b & 31u);
    if (b & 0x60u) return -1; // no other bits
  }
  return 0;
}

extern "C" int host_field_op(int field, int op, const uint32_t* a, const uint32_t* b, uint32_t* out)
{
  switch (field) {
  case 0: return field_op<bn254_fq_params>(op, a, b, out);
  case 1: return field_op<bn254_fr_params>(op, a, b, out);
  case 2: return field_op<bls12_381_fq_params>(op, a, b, out);
  case 3: return field_op<bls12_381_fr_params>(op, a, b, out);
  case 4: return field_op<bls12_377_fq_params>(op, a, b, out);
  case 5: return field_op<bls12_377_fr_params>(op, a, b, out);
  case 6: return field_op<stark252_fr_params>(op, a, b, out);
  case 7: return field_op<goldilocks_params>(op, a, b, out);
  }
  return -1;
}

extern "C" int host_ec_op(int curve, int op, const uint32_t* pts, int n, const uint32_t* aux, uint32_t* out)
{
  switch (curve) {
  case 0: return ec_op<bn254_g1>(op, pts, n, aux, out);
  case 1: return ec_op<bls12_381_g1>(op, pts, n, aux, out);
  case 2: return ec_op<bn254_g2>(op, pts, n, aux, out);
  case 3: return ec_op<bls12_381_g2>(op, pts, n, aux, out);
  case 4: return ec_op<bls12_377_g1>(op, pts, n, aux, out);
  case 5: return ec_op<grumpkin_g1>(op, pts, n, aux, out);
  case 6: return ec_op<bls12_377_g2>(op, pts, n, aux, out);
  }
  return -1;
}

// 31-bit fields
extern "C" int host_small_op(int field, int op, uint32_t a, uint32_t b, uint32_t* out)
{
  if (op < 0 || op > 4) return -1;
  switch (field) {
  case 0: return math_cases::small_case<babybear_params>(op, a, b, out);
  case 1: return math_cases::small_case<koalabear_params>(op, a, b, out);
  }
  return -1;
}

// ---- batched twins of the device harness's entry points (tests/device_math_harness.hip): same arguments, same case bodies,
// one tuple after the other on the host, the bound tracker asserting every precondition ----------------------------------------
extern "C" int host_field_canon(int field, int op, int n, const uint32_t* a, const uint32_t* b, const uint32_t* c, const uint32_t* d, uint32_t* out)
{
  return math_cases::with_field(field, [&](auto tag) {
    using F = typename decltype(tag)::type;
    constexpr size_t W = F::N32;
    for (size_t t = 0; t < (size_t)n; t++)
      if (int e = math_cases::field_case<F>(op, a + t * W, b + t * W, c + t * W, d + t * W, out + t * W)) return e;
    return 0;
  });
}

extern "C" int host_field_raw(int field, int op, int K, const int* kb, int n, const uint32_t* a, const uint32_t* b, const uint32_t* c, const uint32_t* d,
                              uint32_t* out)
{
  return math_cases::with_raw_field(field, [&](auto tag) {
    using F = typename decltype(tag)::type;
    if constexpr (math_cases::is_gold<F>::value || F::N32 > F::N) {
      return -1;
    } else {
      constexpr size_t N = F::N;
      for (size_t t = 0; t < (size_t)n; t++)
        if (int e = math_cases::raw_case<F>(op, K, kb, a + t * N, b + t * N, c + t * N, d + t * N, out + t * N)) return e;
      return 0;
    }
  });
}

extern "C" int host_small_batch(int field, int op, int n, const uint32_t* a, const uint32_t* b, uint32_t* out)
{
  for (int t = 0; t < n; t++) {
    int e = field == 0 ? math_cases::small_case<babybear_params>(op, a[t], b[t], out + t)
                       : (field == 1 ? math_cases::small_case<koalabear_params>(op, a[t], b[t], out + t) : -1);
    if (e) return e;
  }
  return 0;
}

// sequence s holds the points offs[s] .. offs[s+1]-1 (and the aux words of the same indices); 3 * E::N32 words out per sequence
extern "C" int host_ec_batch(int curve, int op, int nseq, const uint32_t* pts, const int* offs, const uint32_t* aux, uint32_t* out)
{
  if (op < 0 || op > 8) return -1; // (ops 7 and 8 answer -1 themselves for the curves that do not have them)
  return math_cases::with_curve(curve, [&](auto tag) {
    using C = typename decltype(tag)::type;
    constexpr size_t N32 = EC<C>::N32;
    for (int s = 0; s < nseq; s++)
      if (int e = math_cases::ec_case<C>(op, pts + (size_t)offs[s] * 2 * N32, offs[s + 1] - offs[s], aux + offs[s], out + (size_t)s * 3 * N32)) return e;
    return 0;
  });
}

// the one-lane twins of the device harness's quad tier on RAW projective operands (math_cases::RawProj limb rows), every component
// with the stated bound K: fn 0 = E::add of two points per case, fn 2 = EcDblSmallB::dbl of one. The tracker aborts the process when
// K is outside a precondition, which is how the tests learn the range the headers' contracts really cover.
extern "C" int host_ec_raw(int curve, int fn, int K, int n, const uint32_t* limbs, uint32_t* out)
{
  return math_cases::with_curve(curve, [&](auto tag) {
    using C = typename decltype(tag)::type;
    const size_t stride = (size_t)(fn == 0 ? 2 : 1) * math_cases::RawProj<C>::ROW;
    for (int t = 0; t < n; t++)
      if (int e = math_cases::ec_raw_case<C>(fn, K, limbs + t * stride, out + (size_t)t * 3 * EC<C>::N32)) return e;
    return 0;
  });
}
