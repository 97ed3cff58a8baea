// The operation code of the element-wise vector kernel: what apply() of every element type in vecops_elem.hpp and
// vecops_ext_elem.hpp switches on. No HIP in here: vecops_ext_elem.hpp is also compiled by plain g++.
#pragma once

namespace icicle_hip {
  enum { VOP_ADD = 0, VOP_SUB = 1, VOP_MUL = 2 };
}
