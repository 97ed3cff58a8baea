// Poseidon2 batch hashing over BabyBear and KoalaBear on the device: the kernels over poseidon2.hpp and the hasher's state. hash.hip
// dispatches to the two launchers below from icicle_hasher_hash and from every Merkle tree path.
//
// One lane hashes one message. A permutation of width 16 over BabyBear is about 770 Montgomery products for 64 bytes read, so the
// work is far on the compute side of the roof and the lanes' strided loads do not matter; what matters is that the state stays in
// registers (tests/test_poseidon2_isa.py) and that the round loop stays rolled: 16 (field, width) pairs times two kernels share the
// instruction cache with the rest of a prover. The round constants are read through a pointer that is the same for every lane, so
// they arrive by scalar loads.
#include "common.h"
#include "poseidon2.hpp"
#include "poseidon2_params.h"
#include <algorithm>

namespace icicle_hip {

  template <class PR, int T>
  __global__ __launch_bounds__(256) void k_poseidon2_batch(const uint8_t* __restrict__ in, uint64_t elems, uint64_t stride, uint64_t n, const Poseidon2Ctx c,
                                                            uint8_t* __restrict__ out)
  {
    const uint64_t step = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += step)
      reinterpret_cast<uint32_t*>(out)[i] = Poseidon2<PR, T>::hash(Poseidon2Words{reinterpret_cast<const uint32_t*>(in + i * stride)}, elems, c);
  }

  template <class PR, int T>
  __global__ __launch_bounds__(256) void k_poseidon2_leaves(const uint8_t* __restrict__ leaves, uint64_t chunk, uint64_t first, uint64_t n, uint64_t valid,
                                                             const uint8_t* __restrict__ last, uint64_t es, const Poseidon2Ctx c, uint8_t* __restrict__ out)
  {
    const uint64_t step = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += step)
      reinterpret_cast<uint32_t*>(out)[i] = Poseidon2<PR, T>::hash(Poseidon2Padded{ReadPadded{leaves, (first + i) * chunk, valid, last, es}}, chunk / 4, c);
  }

  struct Poseidon2Hasher {
    int field = 0;
    unsigned t = 0;
    int half_f = 0, r_p = 0;
    bool has_tag = false;
    uint32_t tag = 0;            // Montgomery
    std::vector<uint32_t> consts; // Montgomery: round constants, then d_i - 1
    std::mutex mtx;
    std::vector<std::pair<int, uint32_t*>> on_device; // (device, copy of consts)
    ~Poseidon2Hasher()
    {
      for (auto& d : on_device)
        (void)hipFree(d.second);
    }
    // the constants on the calling thread's device; the first call per device uploads them, synchronously, so that every stream sees them
    icicle_error_t context(Poseidon2Ctx* c)
    {
      int dev = 0;
      HIP_TRY(hipGetDevice(&dev), ICICLE_INVALID_DEVICE);
      std::lock_guard<std::mutex> lk(mtx);
      const uint32_t* d_consts = nullptr;
      for (auto& d : on_device)
        if (d.first == dev) d_consts = d.second;
      if (!d_consts) {
        uint32_t* buf = nullptr;
        HIP_TRY(hipMalloc((void**)&buf, 4 * consts.size()), ICICLE_ALLOCATION_FAILED);
        if (hipMemcpy(buf, consts.data(), 4 * consts.size(), hipMemcpyHostToDevice) != hipSuccess) {
          (void)hipGetLastError();
          (void)hipFree(buf);
          return ICICLE_COPY_FAILED;
        }
        on_device.emplace_back(dev, buf);
        d_consts = buf;
      }
      *c = Poseidon2Ctx{d_consts, half_f, r_p, tag, has_tag ? 1u : 0u};
      return ICICLE_SUCCESS;
    }
  };

  template <class PR>
  static void poseidon2_fill(Poseidon2Hasher& h, const poseidon2::Params& P, const uint32_t* tag)
  {
    using F = SmallField<PR>;
    h.half_f = P.r_f / 2, h.r_p = P.r_p;
    h.consts = poseidon2_device_constants<PR>(P.rc, P.diag);
    h.has_tag = tag != nullptr;
    h.tag = tag ? F::to_mont(*tag % PR::P) : 0;
  }

  std::shared_ptr<Poseidon2Hasher> poseidon2_make(int field, unsigned t, const uint32_t* tag)
  {
    const uint32_t p = field == 0 ? babybear_params::P : koalabear_params::P;
    const std::shared_ptr<const poseidon2::Params> P = poseidon2::params(p, t);
    if (!P || P->r_f % 2 != 0 || P->alpha != poseidon2_alpha(p)) return nullptr;
    auto h = std::make_shared<Poseidon2Hasher>();
    h->field = field, h->t = t;
    if (field == 0)
      poseidon2_fill<babybear_params>(*h, *P, tag);
    else
      poseidon2_fill<koalabear_params>(*h, *P, tag);
    return h;
  }

  static unsigned poseidon2_grid(uint64_t n) { return (unsigned)std::min<uint64_t>((n + 255) / 256, 1u << 22); }

// one case per width, both fields
#define POSEIDON2_WIDTHS(X) X(2) X(3) X(4) X(8) X(12) X(16) X(20) X(24)

  icicle_error_t poseidon2_launch_batch(Poseidon2Hasher& h, const uint8_t* in, uint64_t len, uint64_t stride, uint64_t n, uint8_t* out, hipStream_t st)
  {
    if (n == 0) return ICICLE_SUCCESS;
    if (len == 0 || (len & 3) || (stride & 3) || ((uintptr_t)in & 3) || ((uintptr_t)out & 3)) return ICICLE_INVALID_ARGUMENT;
    Poseidon2Ctx c;
    ICICLE_TRY(h.context(&c));
    const unsigned grid = poseidon2_grid(n);
    switch (h.t) {
#define POSEIDON2_CASE(T)                                                                                              \
  case T:                                                                                                              \
    if (h.field == 0)                                                                                                  \
      k_poseidon2_batch<babybear_params, T><<<grid, 256, 0, st>>>(in, len / 4, stride, n, c, out);                     \
    else                                                                                                               \
      k_poseidon2_batch<koalabear_params, T><<<grid, 256, 0, st>>>(in, len / 4, stride, n, c, out);                    \
    break;
      POSEIDON2_WIDTHS(POSEIDON2_CASE)
#undef POSEIDON2_CASE
    default: return ICICLE_INVALID_ARGUMENT;
    }
    LAUNCH_CHECK("k_poseidon2_batch", st);
    return ICICLE_SUCCESS;
  }

  icicle_error_t poseidon2_launch_leaves(Poseidon2Hasher& h, const uint8_t* leaves, uint64_t chunk, uint64_t first, uint64_t n, uint64_t valid, const uint8_t* last,
                                         uint64_t es, uint8_t* out, hipStream_t st)
  {
    if (n == 0) return ICICLE_SUCCESS;
    if (chunk == 0 || (chunk & 3) || ((uintptr_t)out & 3)) return ICICLE_INVALID_ARGUMENT;
    Poseidon2Ctx c;
    ICICLE_TRY(h.context(&c));
    const unsigned grid = poseidon2_grid(n);
    switch (h.t) {
#define POSEIDON2_CASE(T)                                                                                              \
  case T:                                                                                                              \
    if (h.field == 0)                                                                                                  \
      k_poseidon2_leaves<babybear_params, T><<<grid, 256, 0, st>>>(leaves, chunk, first, n, valid, last, es, c, out);   \
    else                                                                                                               \
      k_poseidon2_leaves<koalabear_params, T><<<grid, 256, 0, st>>>(leaves, chunk, first, n, valid, last, es, c, out);  \
    break;
      POSEIDON2_WIDTHS(POSEIDON2_CASE)
#undef POSEIDON2_CASE
    default: return ICICLE_INVALID_ARGUMENT;
    }
    LAUNCH_CHECK("k_poseidon2_leaves", st);
    return ICICLE_SUCCESS;
  }

} // namespace icicle_hip
