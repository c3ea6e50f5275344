// nrnerf_field.h -- launch interface of nrnerf_field.hip: the bandwidth-trivial kernels around nrnerf_query (packing the caller's points,
// the detail tensors taken from bent4) and of the grid sampler (nrnerf_grid_points, nrnerf_field_from_raw).  One thread per sample.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace nrn {

// the inputs of a query in the layouts the network kernels read; every output may be nullptr
struct QueryPackArgs {
    const float* points; int stride;     // [N, S, stride >= 3]
    const float* viewdirs;               // [N, 3] or nullptr (zeros)
    long long n_rows; int S;
    float* pts4;                         // [N, S, 4] xyz, 0
    float* init_pts;                     // [N, S, 3] copy of the points (detail tensor initial_input_pts)
    float* in_pts;                       // [N, S, 3] a second copy (input_pts of a model without bender)
    float* records;                      // [N, 11] ray records of the rows: zeros, unit direction (columns 8..10) = viewdirs
    float* point_records;                // [N * S, 11] one ray record per POINT: origin = the point, direction 0, near = far = 0, unit
                                         //   direction = the row's viewdirs -- a "ray" of one sample at depth 0
    float* latents_out; const float* latents; int lat_stride, lat;      // [N * S, lat] the row's latent code per point, or nullptr
};
hipError_t launch_query_pack(const QueryPackArgs& a, hipStream_t stream);

// what a query reports from bent4 [n, 4], and the removal knob on its raw rows (rnh:308-311: sigma * 0 where the mask >= threshold)
struct QueryUnpackArgs {
    const float* bent4; long long n;
    float* in_pts;                       // [n, 3] or nullptr
    float* rigidity;                     // [n] or nullptr
    float* raw; int raw_ch; int has_removal; float removal;      // raw [n, raw_ch] (nullptr / has_removal 0: untouched)
};
hipError_t launch_query_unpack(const QueryUnpackArgs& a, hipStream_t stream);

struct GridArgs {
    float lo[3], hi[3];
    int g[3];                            // gx, gy, gz
    long long first_row; int n_rows;     // rows iz * gy + iy
    float* pts4;                         // [n_rows, gx, 4]
};
hipError_t launch_grid_points(const GridArgs& a, hipStream_t stream);
hipError_t launch_field_from_raw(const float* raw, int raw_ch, long long n, float* sigma, uint8_t* rgb8, hipStream_t stream);

}  // namespace nrn
