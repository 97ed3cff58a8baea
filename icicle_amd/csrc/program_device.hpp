// What sumcheck.hip and execute_program.hip share: the two kinds of field behind one interface, and the object behind a program handle.
#pragma once
#include "common.h"
#include "smallfield.hpp"
#include "bigfield.hpp"
#include "program_lower.h"
#include <mutex>

namespace icicle_hip {

#define SC_D __device__ __forceinline__
#define SC_HD __host__ __device__ __forceinline__

  // ---- the two kinds of field behind one interface: elem = what a lane holds, W = words of an element in memory ----
  template <class PR>
  struct ScSmall {
    using S = SmallField<PR>;
    using elem = uint32_t;
    static constexpr int W = 1, REGS = 1;
    static SC_HD elem zero() { return 0; }
    static SC_HD elem add(elem a, elem b) { return S::add(a, b); }
    static SC_HD elem sub(elem a, elem b) { return S::sub(a, b); }
    static SC_HD elem mul(elem a, elem b) { return S::mul(a, b); } // a b / R
    static SC_HD elem inv(elem a) { return S::inv(a); }            // Montgomery in and out; 0 gives 0
    static constexpr int MONT_BITS = 32;                           // R = 2^32
    static SC_HD elem r2() { return PR::R2; }
    static SC_HD elem mont_one() { return PR::ONE; }
    static SC_HD elem plain_one() { return 1; }
    static SC_HD elem load(const uint32_t* w) { return w[0]; }
    static SC_HD void store(uint32_t* w, elem a) { w[0] = a; }
    static SC_HD uint32_t& reg(elem& a, int) { return a; }
    static HostField host_field()
    {
      const uint32_t p = PR::P;
      return HostField(&p, 1);
    }
  };
  // values below 4p between operations (lazy reduction, bigfield.hpp): a product of two such is below 1.25p
  template <class PR>
  struct ScBig {
    using F = FieldOps<PR>;
    using elem = Fe<PR>;
    static constexpr int W = 8, REGS = PR::NL;
    static SC_HD elem zero() { return F::zero(); }
    static SC_HD elem add(const elem& a, const elem& b)
    {
      elem r = F::add(a, b);
      F::template cond_sub<4>(r);
      return r;
    }
    static SC_HD elem sub(const elem& a, const elem& b)
    {
      elem r = F::template sub<4>(a, b);
      F::template cond_sub<4>(r);
      return r;
    }
    static SC_HD elem mul(const elem& a, const elem& b) { return F::mul(a, b); }
    static SC_HD elem inv(const elem& a) { return F::inv(a); } // Montgomery in and out; 0 gives 0
    static constexpr int MONT_BITS = RB * PR::NL;              // R = 2^(29 * 9)
    static SC_HD elem r2() { return F::r2(); }
    static SC_HD elem mont_one() { return F::one(); }
    static SC_HD elem plain_one() { return F::plain_one(); }
    static SC_HD elem load(const uint32_t* w) { return F::unpack(w); }
    static SC_HD void store(uint32_t* w, const elem& a) { F::pack(w, F::reduce(a)); }
    static SC_HD uint32_t& reg(elem& a, int i) { return a.l[i]; }
    static HostField host_field() { return HostField(PR::P32, 8); }
  };
  template <class PR>
  struct ScFieldOf;
  template <>
  struct ScFieldOf<babybear_params> {
    using type = ScSmall<babybear_params>;
  };
  template <>
  struct ScFieldOf<koalabear_params> {
    using type = ScSmall<koalabear_params>;
  };
  template <>
  struct ScFieldOf<bn254_fr_params> {
    using type = ScBig<bn254_fr_params>;
  };
  template <>
  struct ScFieldOf<bls12_381_fr_params> {
    using type = ScBig<bls12_381_fr_params>;
  };

  // Behind icicle_program_handle_t, for both kinds of program. execute_program lowers the program on its first call and keeps the
  // lowered list and the constants in device memory for the later ones (execute_program.hip).
  struct ProgramObj {
    int words = 0; // of the field it was made for
    CompiledProgram prog;
    std::mutex mtx;        // guards what follows
    int lower_state = -1;  // -1: not lowered yet, else program_lower's result
    LoweredProgram lowered;
    void* d_code = nullptr; // the code words, then the constants as the kernel holds them
    int d_device = -1;
    ProgramObj() = default;
    ProgramObj(const ProgramObj&) = delete;
    ProgramObj& operator=(const ProgramObj&) = delete;
    ~ProgramObj()
    {
      if (d_code) (void)hipFree(d_code);
    }
  };

} // namespace icicle_hip
