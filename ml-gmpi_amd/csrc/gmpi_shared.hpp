// gmpi_shared.hpp -- kernel-side view of the shared-colour layout (GmpiSharedColor, include/gmpi_render.h): what gmpi_abi.hip hands render_shared.hip.
#pragma once
#include <stdint.h>

namespace gmpi {

struct SharedK {
    const void* rgb;   // [M,3,Ht,Wt]
    const void* bg;    // [M,3,Ht,Wt] or nullptr: colour of plane D-1
    int64_t rs_mpi, rs_chan, rs_row, bs_mpi, bs_chan, bs_row;
};
struct SharedG {
    const float* g_out;    // [N,3,H,W]
    const float* g_depth;  // [N,1,H,W] or nullptr
    const float* g_T;      // [N,1,H,W] or nullptr
    float* g_rgb;          // [M,3,Ht,Wt] or nullptr, added into
    float* g_alpha;        // [M,D,1,Ht,Wt] or nullptr
    float* g_bg;           // [M,3,Ht,Wt] or nullptr
    int64_t gr_mpi, gr_chan, gr_row, ga_mpi, ga_plane, ga_row, gb_mpi, gb_chan, gb_row;
};

}  // namespace gmpi
