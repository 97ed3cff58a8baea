// Poseidon2 batch hashing over Goldilocks on the device: the kernels over poseidon2_gold.hpp and the hasher's state. hash.hip
// dispatches to the two launchers below from icicle_hasher_hash and from every Merkle tree path.
//
// One lane hashes one message, 256 lanes per block, as poseidon2.hip. A permutation is 4 T R_F + (4 + T) R_P products of 64 x 64 ->
// 128 bits, 520 at width 8 and 736 at width 12, for 64 or 96 bytes read: the work is far on the compute side of the roof and the
// lanes' strided loads do not matter. What matters is that the state stays in registers (tests/test_poseidon2_gold_isa.py;
// profiles/poseidon2_notes.md has the register counts and the measured rates) and that the round loop stays rolled. The constants
// are read through a pointer that is the same for every lane, so they arrive by scalar loads.
#include "common.h"
#include "poseidon2_gold.hpp"
#include "poseidon2_gold_params.h"
#include <algorithm>

namespace icicle_hip {

  template <int T>
  __global__ __launch_bounds__(256) void k_poseidon2_gold_batch(const uint8_t* __restrict__ in, uint64_t elems, uint64_t stride, uint64_t n, const Poseidon2GoldCtx c,
                                                                 uint8_t* __restrict__ out)
  {
    const uint64_t step = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += step)
      reinterpret_cast<uint64_t*>(out)[i] = Poseidon2Gold<T>::hash(Poseidon2GoldWords{in + i * stride}, elems, c);
  }

  template <int T>
  __global__ __launch_bounds__(256) void k_poseidon2_gold_leaves(const uint8_t* __restrict__ leaves, uint64_t chunk, uint64_t first, uint64_t n, uint64_t valid,
                                                                  const uint8_t* __restrict__ last, uint64_t es, const Poseidon2GoldCtx c, uint8_t* __restrict__ out)
  {
    const uint64_t step = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += step)
      reinterpret_cast<uint64_t*>(out)[i] = Poseidon2Gold<T>::hash(Poseidon2GoldPadded{ReadPadded{leaves, (first + i) * chunk, valid, last, es}}, chunk / 8, c);
  }

  struct Poseidon2GoldHasher {
    unsigned t = 0;
    int half_f = 0, r_p = 0;
    bool has_tag = false;
    uint64_t tag = 0;             // canonical
    std::vector<uint64_t> consts; // canonical: round constants, then d_i - 1
    std::mutex mtx;
    std::vector<std::pair<int, uint64_t*>> on_device; // (device, copy of consts)
    ~Poseidon2GoldHasher()
    {
      for (auto& d : on_device)
        (void)hipFree(d.second);
    }
    // the constants on the calling thread's device; the first call per device uploads them, synchronously, so that every stream sees them
    icicle_error_t context(Poseidon2GoldCtx* c)
    {
      int dev = 0;
      HIP_TRY(hipGetDevice(&dev), ICICLE_INVALID_DEVICE);
      std::lock_guard<std::mutex> lk(mtx);
      const uint64_t* d_consts = nullptr;
      for (auto& d : on_device)
        if (d.first == dev) d_consts = d.second;
      if (!d_consts) {
        uint64_t* buf = nullptr;
        HIP_TRY(hipMalloc((void**)&buf, 8 * consts.size()), ICICLE_ALLOCATION_FAILED);
        if (hipMemcpy(buf, consts.data(), 8 * consts.size(), hipMemcpyHostToDevice) != hipSuccess) {
          (void)hipGetLastError();
          (void)hipFree(buf);
          return ICICLE_COPY_FAILED;
        }
        on_device.emplace_back(dev, buf);
        d_consts = buf;
      }
      *c = Poseidon2GoldCtx{d_consts, half_f, r_p, tag, has_tag ? 1u : 0u};
      return ICICLE_SUCCESS;
    }
  };

  // nullptr where the derived parameters are not what the lane code is compiled for: x^7 and an even R_F
  std::shared_ptr<Poseidon2GoldHasher> poseidon2_gold_make(unsigned t, const uint32_t* tag)
  {
    const uint64_t tag_value = tag ? (uint64_t)tag[0] | (uint64_t)tag[1] << 32 : 0;
    if (tag_value >= goldilocks_params::P) return nullptr;
    const std::shared_ptr<const poseidon2_gold::Params> P = poseidon2_gold::params(t);
    if (!P || P->r_f % 2 != 0 || P->alpha != 7) return nullptr;
    auto h = std::make_shared<Poseidon2GoldHasher>();
    h->t = t, h->half_f = P->r_f / 2, h->r_p = P->r_p;
    h->consts = poseidon2_gold_device_constants(P->rc, P->diag);
    h->has_tag = tag != nullptr, h->tag = tag_value;
    return h;
  }

  static unsigned poseidon2_gold_grid(uint64_t n) { return (unsigned)std::min<uint64_t>((n + 255) / 256, 1u << 22); }

// one case per width
#define POSEIDON2_GOLD_WIDTHS(X) X(2) X(3) X(4) X(8) X(12) X(16) X(20) X(24)

  icicle_error_t poseidon2_gold_launch_batch(Poseidon2GoldHasher& h, const uint8_t* in, uint64_t len, uint64_t stride, uint64_t n, uint8_t* out, hipStream_t st)
  {
    if (n == 0) return ICICLE_SUCCESS;
    if (len == 0 || (len & 7) || stride == 0 || (stride & 7) || ((uintptr_t)in & 7) || ((uintptr_t)out & 7)) return ICICLE_INVALID_ARGUMENT;
    Poseidon2GoldCtx c;
    ICICLE_TRY(h.context(&c));
    const unsigned grid = poseidon2_gold_grid(n);
    switch (h.t) {
#define POSEIDON2_GOLD_CASE(T)                                                                                         \
  case T: k_poseidon2_gold_batch<T><<<grid, 256, 0, st>>>(in, len / 8, stride, n, c, out); break;
      POSEIDON2_GOLD_WIDTHS(POSEIDON2_GOLD_CASE)
#undef POSEIDON2_GOLD_CASE
    default: return ICICLE_INVALID_ARGUMENT;
    }
    LAUNCH_CHECK("k_poseidon2_gold_batch", st);
    return ICICLE_SUCCESS;
  }

  icicle_error_t poseidon2_gold_launch_leaves(Poseidon2GoldHasher& h, const uint8_t* leaves, uint64_t chunk, uint64_t first, uint64_t n, uint64_t valid,
                                              const uint8_t* last, uint64_t es, uint8_t* out, hipStream_t st)
  {
    if (n == 0) return ICICLE_SUCCESS;
    if (chunk == 0 || (chunk & 7) || ((uintptr_t)out & 7)) return ICICLE_INVALID_ARGUMENT;
    Poseidon2GoldCtx c;
    ICICLE_TRY(h.context(&c));
    const unsigned grid = poseidon2_gold_grid(n);
    switch (h.t) {
#define POSEIDON2_GOLD_CASE(T)                                                                                         \
  case T: k_poseidon2_gold_leaves<T><<<grid, 256, 0, st>>>(leaves, chunk, first, n, valid, last, es, c, out); break;
      POSEIDON2_GOLD_WIDTHS(POSEIDON2_GOLD_CASE)
#undef POSEIDON2_GOLD_CASE
    default: return ICICLE_INVALID_ARGUMENT;
    }
    LAUNCH_CHECK("k_poseidon2_gold_leaves", st);
    return ICICLE_SUCCESS;
  }

} // namespace icicle_hip
