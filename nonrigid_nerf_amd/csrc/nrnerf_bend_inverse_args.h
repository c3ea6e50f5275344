// nrnerf_bend_inverse_args.h -- launch interface of the inverse bender (the kernel: nrnerf_bend_inverse.h; what nrnerf_bender_inverse runs).
// No kernel body: the entry point's unit includes this alone.
#pragma once
#include "nrnerf_kernels.h"

namespace nrn {

struct BendInverseArgs {
    const float* canonical; int stride;   // [n_rows, n_per_row, stride >= 3]; 16-byte loads when stride == 4 and the base is 16-byte aligned
    const float* initial;                 // [n_rows, n_per_row, stride] first guess, or nullptr: the canonical point
    const float* latents; int lat_stride; // per row; 0: one code for the launch
    int n_rows, n_per_row;
    const void* wstream;                  // the image the point-source fp32 bender reads (Plan<PolF32, A, true, false, false>)
    const float* bias;
    Knobs knobs;                          // has_cutoff / cutoff, has_scaling / scaling: part of the map that is inverted
    float tol, omega;
    int max_iters;                        // >= 1
    float* observed;                      // out [n_rows, n_per_row, 3]
    float* residual;                      // out [n_rows, n_per_row] max_c |bend(observed)_c - canonical_c|, or nullptr
    int* iterations;                      // out [n_rows, n_per_row] evaluations made, 1 .. max_iters, or nullptr
    unsigned* work_counter;               // a device counter, ZERO at launch, or nullptr: fixed shares
};
// bender architectures 0 (5 x 64) and 1 (7 x 64); hipErrorInvalidValue for another one or for 2^31 or more blocks (nothing is launched)
hipError_t launch_bend_inverse(int bender_arch, const BendInverseArgs& a, int num_cus, hipStream_t stream);

}  // namespace nrn
