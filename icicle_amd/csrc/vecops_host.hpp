// The host frame of every vector operation: an operand staged onto the device (Staged) and a result staged off it (StagedOut).
// A run function validates its arguments, binds the device, stages its operands and its result, launches on `dev` and finishes.
#pragma once
#include "common.h"

namespace icicle_hip {

  struct Staged { // host <-> device staging of one operand
    TempBuf buf;
    const uint32_t* dev = nullptr;
    icicle_error_t in(const void* p, bool on_device, size_t bytes, hipStream_t st)
    {
      if (on_device) {
        dev = (const uint32_t*)p;
        return ICICLE_SUCCESS;
      }
      HIP_TRY(buf.alloc(bytes, st), ICICLE_ALLOCATION_FAILED);
      HIP_TRY(hipMemcpyAsync(buf.ptr(), p, bytes, hipMemcpyHostToDevice, st), ICICLE_COPY_FAILED);
      dev = buf.as<uint32_t>();
      return ICICLE_SUCCESS;
    }
  };

  struct StagedOut { // device <-> host staging of one result
    TempBuf buf;
    uint32_t* dev = nullptr; // what the kernels write

    // A result on the host, or one on the device at `alias` -- the device input of a kernel that cannot run in place -- is written to
    // a temporary and copied to its place by finish(); any other device result is written where the caller wants it.
    icicle_error_t out(void* p, bool on_device, size_t bytes, hipStream_t st, const void* alias = nullptr)
    {
      adopt(p, on_device, bytes, st, (uint32_t*)p);
      if (on_device && p != alias) return ICICLE_SUCCESS;
      HIP_TRY(buf.alloc(bytes, st), ICICLE_ALLOCATION_FAILED);
      dev = buf.as<uint32_t>();
      return ICICLE_SUCCESS;
    }
    // the same with a device buffer the caller of this already holds (the staging buffer of an operand that is updated in place)
    void adopt(void* p, bool on_device, size_t bytes, hipStream_t st, uint32_t* d)
    {
      m_p = p, m_on_device = on_device, m_bytes = bytes, m_st = st, dev = d;
    }

    icicle_error_t copy_back() // issues the copy to the caller's place, where there is one to make
    {
      if (dev == m_p || m_bytes == 0) return ICICLE_SUCCESS;
      HIP_TRY(hipMemcpyAsync(m_p, dev, m_bytes, m_on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, m_st), ICICLE_COPY_FAILED);
      return ICICLE_SUCCESS;
    }
    // a host result is complete on return; a device result unless the call is asynchronous. Several results of one call: copy_back()
    // on all but the last, whose finish() synchronises for all of them.
    icicle_error_t finish(bool is_async)
    {
      ICICLE_TRY(copy_back());
      if (!m_on_device || !is_async) HIP_TRY(hipStreamSynchronize(m_st), ICICLE_SYNCHRONIZATION_FAILED);
      return ICICLE_SUCCESS;
    }

  private:
    void* m_p = nullptr;
    bool m_on_device = false;
    size_t m_bytes = 0;
    hipStream_t m_st = nullptr;
  };

} // namespace icicle_hip
