// TEST-ONLY device twin of tests/host_math_harness.cpp: kernels that run ONE operand tuple per thread through the case bodies of
// math_cases.hpp, i.e. through the same header calls as the host harness -- but compiled for gfx950, where FieldOps::mul / sqr /
// mul_add / mul_inplace / mul_add_inplace_c of the 9- and 14-limb fields are the inline-asm blocks of mont_asm.hpp and goldilocks
// multiplies with __umul64hi. Built twice with the product's flags (tests/device_math.mk): as shipped (libdevice_math_asm.so) and
// with -DBIGFIELD_NO_ASM (libdevice_math_noasm.so). The C entry points take HOST arrays, stage them themselves and return the HIP
// error code (0 = success; -1 = unknown field / op, nothing launched).
//
// Both libraries are loaded into one process: every kernel has internal linkage inside a per-variant namespace, everything but the
// entry points is hidden (-fvisibility=hidden), and every launch writes the compiled-in variant tag next to its results so that the
// tests can tell which build really produced them. Nothing here names or loads the oracle or any reference code: the expected
// values are Python integers.
#include <hip/hip_runtime.h>
#include "math_cases.hpp"

#ifdef BIGFIELD_NO_ASM
  #define DM_NS dm_noasm
  #define DM_TAG 0x4e4f4153u // "NOAS"
#else
  #define DM_NS dm_asm
  #define DM_TAG 0x41534d31u // "ASM1"
#endif
#define DM_EXPORT extern "C" __attribute__((visibility("default")))

namespace DM_NS {
  namespace {
    using namespace icicle_hip;
    constexpr int BLOCK = 64;

    __device__ __forceinline__ void put_tag(uint32_t* tag)
    {
      if (blockIdx.x == 0 && threadIdx.x == 0) *tag = DM_TAG;
    }

    template <class F>
    __global__ __launch_bounds__(BLOCK) void k_field(int op, int n, const uint32_t* a, const uint32_t* b, const uint32_t* c, const uint32_t* d, uint32_t* out,
                                                     uint32_t* tag, int* bad)
    {
      put_tag(tag);
      const size_t t = (size_t)blockIdx.x * BLOCK + threadIdx.x;
      if (t >= (size_t)n) return;
      constexpr size_t W = F::N32;
      if (math_cases::field_case<F>(op, a + t * W, b + t * W, c + t * W, d + t * W, out + t * W)) *bad = 1;
    }

    template <class F>
    __global__ __launch_bounds__(BLOCK) void k_raw(int op, int K, int k0, int k1, int k2, int k3, int n, const uint32_t* a, const uint32_t* b, const uint32_t* c,
                                                   const uint32_t* d, uint32_t* out, uint32_t* tag, int* bad)
    {
      put_tag(tag);
      const size_t t = (size_t)blockIdx.x * BLOCK + threadIdx.x;
      if (t >= (size_t)n) return;
      constexpr size_t N = F::N;
      const int kb[4] = {k0, k1, k2, k3};
      if (math_cases::raw_case<F>(op, K, kb, a + t * N, b + t * N, c + t * N, d + t * N, out + t * N)) *bad = 1;
    }

    template <class PR>
    __global__ __launch_bounds__(BLOCK) void k_small(int op, int n, const uint32_t* a, const uint32_t* b, uint32_t* out, uint32_t* tag, int* bad)
    {
      put_tag(tag);
      const size_t t = (size_t)blockIdx.x * BLOCK + threadIdx.x;
      if (t >= (size_t)n) return;
      if (math_cases::small_case<PR>(op, a[t], b[t], out + t)) *bad = 1;
    }

    template <class C>
    __global__ __launch_bounds__(BLOCK) void k_ec(int op, int nseq, const uint32_t* pts, const int* offs, const uint32_t* aux, uint32_t* out, uint32_t* tag, int* bad)
    {
      put_tag(tag);
      const size_t s = (size_t)blockIdx.x * BLOCK + threadIdx.x;
      if (s >= (size_t)nseq) return;
      constexpr size_t N32 = EC<C>::N32;
      if (math_cases::ec_case<C>(op, pts + (size_t)offs[s] * 2 * N32, offs[s + 1] - offs[s], aux + offs[s], out + s * 3 * N32)) *bad = 1;
    }

    // ---- quad tier: the four-lane EC operations (ec.hpp add_quad / dbl_jac_quad, ec_dbl_quad.hpp EcQuadAdd::add / dbl_quad), which no
    // host build reaches. One SEQUENCE PER DPP QUAD: a block of 64 threads holds 16 quads, role = threadIdx.x & 3 is the physical lane
    // number mod 4, all four lanes of a quad load the same operands and run the same chain, and EVERY lane stores its own canonical
    // result at out[(seq * 4 + role) * 3 * N32] (lanes 1..3 feed the next operation of every real chain). The kernel diverges at
    // quad granularity only -- sequence lengths and doubling counts differ per quad, quads past nseq return -- as the product's
    // kernels do. One instantiation per (curve, op) the product has; nothing else is compiled.
    //   OP 0: complete sum with EcQuadAdd::add from proj_identity(); aux & 1 negates, (0, 0) is the identity   (ec_case op 1's twin)
    //   OP 1: the same with EC::add_quad
    //   OP 2: 2^aux[0] * pts[0] by dbl_quad, the point given a non-trivial Z by an addition of the identity    (ec_case op 8's twin)
    //   OP 3: to_jac, aux[0] x dbl_jac_quad, from_jac                                                          (ec_case op 5's twin)
    //   OP 4: the Horner walk of k_final_horner, branch for branch: acc = 2^(aux[i] >> 1) * acc + (-1)^(aux[i] & 1) pts[i], i = 1 ..;
    //         acc and every addend come out of a quad addition, so each operand carries the bound the previous op really leaves
    //   RAW (OP 0: two points per sequence, OP 2: one point, one doubling): the operands are math_cases::RawProj limb rows
    template <class C>
    inline constexpr bool has_quad_add = C::EXT_DEGREE == 1 || std::is_same<C, bn254_g2>::value; // k_reduce_*_quad: G1 and BN254 G2
    template <class C, int OP>
    inline constexpr bool has_quad_op = OP == 0 ? has_quad_add<C> : OP == 2 ? has_small_b3<C>::value : OP == 4 ? true : !has_small_b3<C>::value;

    template <class C, int OP, bool RAW>
    __global__ __launch_bounds__(BLOCK) void k_ec_quad(int nseq, const uint32_t* pts, const int* offs, const uint32_t* aux, uint32_t* out, uint32_t* tag)
    {
      put_tag(tag);
      using E = EC<C>;
      using F = typename E::F;
      using Proj = typename E::Proj;
      constexpr size_t N32 = E::N32;
      const uint32_t role = threadIdx.x & 3u;
      const size_t s = (size_t)blockIdx.x * (BLOCK / 4) + (threadIdx.x >> 2);
      if (s >= (size_t)nseq) return; // whole quads only
      const int o0 = offs[s], n = offs[s + 1] - o0;
      auto is_identity = [&](int i) { return E::words_are_zero(pts + (size_t)(o0 + i) * 2 * N32); };
      auto point = [&](int i, bool signed_aux = true) { // pts[i] as a projective operand, negated when aux & 1 says so; (0, 0) = the identity
        const uint32_t* w = pts + (size_t)(o0 + i) * 2 * N32;
        typename E::Aff a;
        a.x = F::from_canonical(w);
        a.y = F::from_canonical(w + N32);
        return is_identity(i) ? E::proj_identity() : E::to_proj(E::cneg(a, signed_aux && (aux[o0 + i] & 1u) != 0));
      };
      auto qadd = [&](const Proj& a, const Proj& b) { // the complete addition the product pairs with this op on this curve
        if constexpr (OP == 0 || (OP != 1 && has_small_b3<C>::value))
          return EcQuadAdd<C>::add(a, b, role);
        else
          return E::add_quad(a, b, role);
      };
      Proj r;
      if constexpr (RAW) {
        using RP = math_cases::RawProj<C>;
        const uint32_t* l = pts + (size_t)o0 * RP::ROW;
        if constexpr (OP == 0)
          r = EcQuadAdd<C>::add(RP::load(l, 0), RP::load(l + RP::ROW, 0), role);
        else
          r = EcDblSmallB<C>::dbl_quad(RP::load(l, 0), role);
      } else if constexpr (OP == 0 || OP == 1) {
        r = E::proj_identity();
        for (int i = 0; i < n; i++)
          r = qadd(r, point(i));
      } else if constexpr (OP == 2 || OP == 3) {
        r = qadd(point(0, false), E::proj_identity()); // a non-trivial Z (aux[0] is the doubling count)
        if (is_identity(0)) r = E::proj_identity(); // (as the one-lane twins start)
        const uint32_t k = aux[o0];
        if constexpr (OP == 2) {
          for (uint32_t i = 0; i < k; i++)
            r = EcDblSmallB<C>::dbl_quad(r, role);
        } else {
          typename E::Jac j = E::to_jac(r);
          for (uint32_t i = 0; i < k; i++)
            j = E::dbl_jac_quad(j, role);
          r = E::from_jac(j);
        }
      } else {
        r = E::proj_identity();
        for (int i = 0; i < n; i++) {
          const Proj sw = qadd(E::proj_identity(), point(i)); // a window sum as a quad addition leaves it
          if (i == 0) {
            r = sw;
            continue;
          }
          const int nd = (int)(aux[o0 + i] >> 1);
          if constexpr (has_small_b3<C>::value) {
            for (int q = 0; q < nd; q++)
              r = EcDblSmallB<C>::dbl_quad(r, role);
            r = EcQuadAdd<C>::add(r, sw, role);
          } else {
            typename E::Jac j = E::to_jac(r);
            for (int q = 0; q < nd; q++)
              j = E::dbl_jac_quad(j, role);
            r = E::add_quad(E::from_jac(j), sw, role);
          }
        }
      }
      E::store_proj_canonical(out + (s * 4 + role) * 3 * N32, r);
    }

    // host side: device copies of the host arrays, freed on every path
    struct Staged {
      static constexpr int MAX = 10;
      void* p[MAX];
      int cnt = 0;
      hipError_t err = hipSuccess;
      template <class T>
      T* in(const T* h, size_t count)
      {
        T* dp = out<T>(count);
        if (err == hipSuccess && count) err = hipMemcpy(dp, h, count * sizeof(T), hipMemcpyHostToDevice);
        return dp;
      }
      template <class T>
      T* out(size_t count)
      {
        void* dp = nullptr;
        if (err == hipSuccess && cnt < MAX) {
          err = hipMalloc(&dp, (count ? count : 1) * sizeof(T));
          if (err == hipSuccess) {
            p[cnt++] = dp;
            err = hipMemset(dp, 0, (count ? count : 1) * sizeof(T));
          }
        }
        return (T*)dp;
      }
      template <class T>
      void back(T* h, const T* dp, size_t count)
      {
        if (err == hipSuccess) err = hipDeviceSynchronize();
        if (err == hipSuccess && count) err = hipMemcpy(h, dp, count * sizeof(T), hipMemcpyDeviceToHost);
      }
      void launched()
      {
        if (err == hipSuccess) err = hipGetLastError();
      }
      ~Staged()
      {
        for (int i = 0; i < cnt; i++)
          (void)hipFree(p[i]);
      }
    };
    inline int finish(Staged& st, const int* d_bad)
    {
      int bad = 0;
      st.back(&bad, d_bad, 1);
      if (st.err != hipSuccess) return (int)st.err;
      return bad ? -1 : 0;
    }
  } // namespace
} // namespace DM_NS

using namespace DM_NS;

// the variant this library was compiled as (host-side constant; the kernels write the same tag from device code)
DM_EXPORT uint32_t dm_variant_tag() { return DM_TAG; }

// canonical mode: n tuples of F::N32 words per operand; out: n * F::N32 words; tag: one word written by the kernel
DM_EXPORT int dm_field_canon(int field, int op, int n, const uint32_t* a, const uint32_t* b, const uint32_t* c, const uint32_t* d, uint32_t* out, uint32_t* tag)
{
  if (n <= 0) return -1;
  return math_cases::with_field(field, [&](auto t) {
    using F = typename decltype(t)::type;
    const size_t cnt = (size_t)n * F::N32;
    Staged st;
    auto da = st.in(a, cnt), db = st.in(b, cnt), dc = st.in(c, cnt), dd = st.in(d, cnt);
    auto dout = st.out<uint32_t>(cnt), dtag = st.out<uint32_t>(1);
    auto dbad = st.out<int>(1);
    if (st.err == hipSuccess) {
      k_field<F><<<(n + BLOCK - 1) / BLOCK, BLOCK>>>(op, n, da, db, dc, dd, dout, dtag, dbad);
      st.launched();
    }
    st.back(out, dout, cnt);
    st.back(tag, dtag, 1);
    return finish(st, dbad);
  });
}

// raw mode (fields 0..6): n tuples of F::N limbs per operand; kb[4] = the stated bounds of a, b, c, d; K = the template argument of
// sub<K> / cond_sub<K>; out: n * F::N limbs
DM_EXPORT int dm_field_raw(int field, int op, int K, const int* kb, int n, const uint32_t* a, const uint32_t* b, const uint32_t* c, const uint32_t* d, uint32_t* out,
                           uint32_t* tag)
{
  if (n <= 0) return -1;
  return math_cases::with_raw_field(field, [&](auto t) {
    using F = typename decltype(t)::type;
    if constexpr (math_cases::is_gold<F>::value || F::N32 > F::N) {
      return -1;
    } else {
      const size_t cnt = (size_t)n * F::N;
      Staged st;
      auto da = st.in(a, cnt), db = st.in(b, cnt), dc = st.in(c, cnt), dd = st.in(d, cnt);
      auto dout = st.out<uint32_t>(cnt), dtag = st.out<uint32_t>(1);
      auto dbad = st.out<int>(1);
      if (st.err == hipSuccess) {
        k_raw<F><<<(n + BLOCK - 1) / BLOCK, BLOCK>>>(op, K, kb[0], kb[1], kb[2], kb[3], n, da, db, dc, dd, dout, dtag, dbad);
        st.launched();
      }
      st.back(out, dout, cnt);
      st.back(tag, dtag, 1);
      return finish(st, dbad);
    }
  });
}

// 31-bit fields (0 BabyBear, 1 KoalaBear): canonical residues
DM_EXPORT int dm_small(int field, int op, int n, const uint32_t* a, const uint32_t* b, uint32_t* out, uint32_t* tag)
{
  if (n <= 0 || field < 0 || field > 1) return -1;
  Staged st;
  auto da = st.in(a, n), db = st.in(b, n);
  auto dout = st.out<uint32_t>(n), dtag = st.out<uint32_t>(1);
  auto dbad = st.out<int>(1);
  if (st.err == hipSuccess) {
    if (field == 0)
      k_small<babybear_params><<<(n + BLOCK - 1) / BLOCK, BLOCK>>>(op, n, da, db, dout, dtag, dbad);
    else
      k_small<koalabear_params><<<(n + BLOCK - 1) / BLOCK, BLOCK>>>(op, n, da, db, dout, dtag, dbad);
    st.launched();
  }
  st.back(out, dout, n);
  st.back(tag, dtag, 1);
  return finish(st, dbad);
}

// EC tier: sequence s = points offs[s] .. offs[s+1]-1 (at least one each; aux words at the same indices); out: nseq * 3 * E::N32 words.
// op 7 (add_signed) only for the curves with SIGNED_MADD, op 8 (EcDblSmallB::dbl) only for those with a small 3 b: -1 otherwise
DM_EXPORT int dm_ec(int curve, int op, int nseq, const uint32_t* pts, const int* offs, const uint32_t* aux, uint32_t* out, uint32_t* tag)
{
  if (nseq <= 0 || op < 0 || op > 8) return -1;
  for (int s = 0; s < nseq; s++)
    if (offs[s + 1] <= offs[s] || offs[s] < 0) return -1;
  return math_cases::with_curve(curve, [&](auto t) {
    using C = typename decltype(t)::type;
    if ((op == 7 && !EC<C>::SIGNED_MADD) || (op == 8 && !has_small_b3<C>::value)) return -1; // (nothing launched)
    constexpr size_t N32 = EC<C>::N32;
    const size_t npts = (size_t)offs[nseq], ocnt = (size_t)nseq * 3 * N32;
    Staged st;
    auto dp = st.in(pts, npts * 2 * N32);
    auto doffs = st.in(offs, (size_t)nseq + 1);
    auto daux = st.in(aux, npts);
    auto dout = st.out<uint32_t>(ocnt), dtag = st.out<uint32_t>(1);
    auto dbad = st.out<int>(1);
    if (st.err == hipSuccess) {
      k_ec<C><<<(nseq + BLOCK - 1) / BLOCK, BLOCK>>>(op, nseq, dp, doffs, daux, dout, dtag, dbad);
      st.launched();
    }
    st.back(out, dout, ocnt);
    st.back(tag, dtag, 1);
    return finish(st, dbad);
  });
}

// quad tier (k_ec_quad): op = 0..4, | 0x100 for raw limb-row operands (ops 0 and 2 only: exactly two points / one point per sequence).
// pts: affine canonical words as for dm_ec, or RawProj rows; out: nseq * 4 * 3 * E::N32 words, one result per lane of every quad.
// -1 (nothing launched) for a (curve, op) pair the product does not instantiate.
namespace DM_NS {
  namespace {
    template <class C, int OP, bool RAW>
    int run_ec_quad(int nseq, const uint32_t* pts, const int* offs, const uint32_t* aux, uint32_t* out, uint32_t* tag)
    {
      if constexpr (!has_quad_op<C, OP>) {
        return -1;
      } else {
        constexpr size_t N32 = EC<C>::N32;
        const size_t npts = (size_t)offs[nseq], ocnt = (size_t)nseq * 4 * 3 * N32;
        Staged st;
        auto dp = st.in(pts, npts * (RAW ? (size_t)math_cases::RawProj<C>::ROW : 2 * N32));
        auto doffs = st.in(offs, (size_t)nseq + 1);
        auto daux = st.in(aux, npts);
        auto dout = st.out<uint32_t>(ocnt), dtag = st.out<uint32_t>(1);
        if (st.err == hipSuccess) {
          k_ec_quad<C, OP, RAW><<<(nseq + BLOCK / 4 - 1) / (BLOCK / 4), BLOCK>>>(nseq, dp, doffs, daux, dout, dtag);
          st.launched();
        }
        st.back(out, dout, ocnt);
        st.back(tag, dtag, 1);
        return (int)st.err;
      }
    }
  } // namespace
} // namespace DM_NS

DM_EXPORT int dm_ec_quad(int curve, int op, int nseq, const uint32_t* pts, const int* offs, const uint32_t* aux, uint32_t* out, uint32_t* tag)
{
  const bool raw = (op & 0x100) != 0;
  const int o = op & ~0x100;
  if (nseq <= 0 || o < 0 || o > 4 || (raw && o != 0 && o != 2) || offs[0] != 0) return -1;
  for (int s = 0; s < nseq; s++) {
    const int n = offs[s + 1] - offs[s];
    if (n <= 0 || (raw && n != (o == 0 ? 2 : 1))) return -1;
  }
  return math_cases::with_curve(curve, [&](auto t) {
    using C = typename decltype(t)::type;
    switch (op) {
    case 0: return run_ec_quad<C, 0, false>(nseq, pts, offs, aux, out, tag);
    case 1: return run_ec_quad<C, 1, false>(nseq, pts, offs, aux, out, tag);
    case 2: return run_ec_quad<C, 2, false>(nseq, pts, offs, aux, out, tag);
    case 3: return run_ec_quad<C, 3, false>(nseq, pts, offs, aux, out, tag);
    case 4: return run_ec_quad<C, 4, false>(nseq, pts, offs, aux, out, tag);
    case 0x100: return run_ec_quad<C, 0, true>(nseq, pts, offs, aux, out, tag);
    case 0x102: return run_ec_quad<C, 2, true>(nseq, pts, offs, aux, out, tag);
    }
    return -1;
  });
}
