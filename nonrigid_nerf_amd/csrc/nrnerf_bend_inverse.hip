// nrnerf_bend_inverse.hip -- the instantiations of the inverse bender (nrnerf_bend_inverse.h): fp32, bender architectures 0 (5 x 64) and
// 1 (7 x 64), four waves per workgroup.
#include "nrnerf_bend_inverse.h"

namespace nrn {
hipError_t launch_bend_inverse(int bender_arch, const BendInverseArgs& a, int num_cus, hipStream_t stream) {
    switch (bender_arch) {
        case 0: return launch_bend_inverse_one<ArchById<0>::type, 4>(a, num_cus, stream);
        case 1: return launch_bend_inverse_one<ArchById<1>::type, 4>(a, num_cus, stream);
        default: return hipErrorInvalidValue;
    }
}
}  // namespace nrn
