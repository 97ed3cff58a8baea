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

// EC tier: sequence s = points offs[s] .. offs[s+1]-1 (at least one each; aux words at the same indices); out: nseq * 3 * E::N32 words
DM_EXPORT int dm_ec(int curve, int op, int nseq, const uint32_t* pts, const int* offs, const uint32_t* aux, uint32_t* out, uint32_t* tag)
{
  if (nseq <= 0 || op < 0 || op > 6) return -1;
  for (int s = 0; s < nseq; s++)
    if (offs[s + 1] <= offs[s] || offs[s] < 0) return -1;
  return math_cases::with_curve(curve, [&](auto t) {
    using C = typename decltype(t)::type;
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
