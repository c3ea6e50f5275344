// nrnerf_bend_inst.hip -- one instantiation of the stand-alone bender kernel (nrnerf_bend.h) per translation unit, and of its point-source
// variant (launcher NRN_NAME with `_points` appended).  Build with
//   -DNRN_POL=PolBF16 -DNRN_ARCH=0 -DNRN_NAME=launch_bend_a0_bf16
#include "nrnerf_bend.h"

#define NRN_CAT2(a, b) a##b
#define NRN_CAT(a, b) NRN_CAT2(a, b)

namespace nrn {
hipError_t NRN_NAME(const BendArgs& a, int num_cus, hipStream_t stream) {
    return launch_bend_one<NRN_POL, ArchById<NRN_ARCH>::type, (NRN_POL::KH == 1) ? 4 : 8>(a, num_cus, stream);
}
hipError_t NRN_CAT(NRN_NAME, _points)(const BendPointArgs& a, int num_cus, hipStream_t stream) {
    return launch_bend_one<NRN_POL, ArchById<NRN_ARCH>::type, (NRN_POL::KH == 1) ? 4 : 8>(a, num_cus, stream);
}
}  // namespace nrn
