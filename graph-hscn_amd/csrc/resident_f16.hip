// Graph-resident HSCN engine with IEEE-half storage of node features and inter-layer activations
// (BASELINE.json configs[4]: "fp16 feat + bf16 accum" on PCQM-Contact): the kernels of resident_kernels.h
// instantiated with TS = half_t.  What is half: x_local, x_virtual, acts, xv_out and the job's x_virtual / xv_out /
// st_xv (every array that holds a node feature or an activation in HBM).  What stays float: parameters, pooled, z,
// pred, score, degree norms, gradient partials and gradients -- all sums accumulate in float registers (a superset
// of bf16 accumulation: same exponent range, 16 more mantissa bits).  An activation is rounded to half once, where
// it is produced, in LDS and in HBM alike.  H in {16, 32}.  resident.hip's entry points reach the instantiations
// through the table below (HSCN_STORE_F16).
#include "resident_kernels.h"


bool hscn_resident_f16_takes(int H) { return H == 16 || H == 32; }

// (a function's static, not a namespace-scope constant: the device pass would emit that one as well)
const hscn_resident_f16_table& hscn_resident_f16() {
  static const hscn_resident_f16_table table = {
      impl_resident_fwd<half_t>,
      impl_resident_bwd<half_t>,
      impl_resident_bwd_with_virtual<half_t>,
      impl_resident_fwd_with_virtual<half_t>,
      impl_resident_train_step<half_t>,
  };
  return table;
}
