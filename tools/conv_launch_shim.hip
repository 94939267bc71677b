// Stand-in for the HIP launch calls, for tools/conv_plan_cases.py: loaded (RTLD_GLOBAL) ahead of libegorear_hip.so it takes every
// kernel launch of the library instead of the runtime, notes what would have been launched - host stub, grid, workgroup size and
// the plan-dependent fields of the ConvArgs kernel argument - and launches nothing.  So the launch entry points can be asked what
// they decide with fake pointers, on any machine, at any commit whose ConvArgs this file is compiled against.
#include <dlfcn.h>

#include "egr_conv_shared.h"

namespace {
struct Rec {
    uint64_t stub;               // offset of the kernel's host stub in its shared object
    uint32_t grid[3], block[3];
    int32_t split_k, ktiles_per_split, tiles_m, tiles_n, has_cnt;
};
Rec g_rec[8];
int g_n = 0;
int g_counters[2048 * 64];       // what hipGetSymbolAddress hands out for the split-K arrival counters
}  // namespace

// the two halves of `kernel<<<grid, block, shmem, stream>>>(...)` around the host stub (the runtime's need a device)
namespace {
dim3 g_grid, g_block;
}
extern "C" hipError_t __hipPushCallConfiguration(dim3 grid, dim3 block, size_t, hipStream_t) {
    g_grid = grid; g_block = block;
    return hipSuccess;
}
extern "C" hipError_t __hipPopCallConfiguration(dim3* grid, dim3* block, size_t* shmem, hipStream_t* stream) {
    *grid = g_grid; *block = g_block; *shmem = 0; *stream = nullptr;
    return hipSuccess;
}
extern "C" hipError_t hipLaunchKernel(const void* f, dim3 grid, dim3 block, void** args, size_t, hipStream_t) {
    Dl_info info;
    if (g_n < 8 && dladdr(f, &info)) {
        const egrc::ConvArgs& a = *static_cast<const egrc::ConvArgs*>(args[0]);
        g_rec[g_n++] = {(uint64_t)((const char*)f - (const char*)info.dli_fbase), {grid.x, grid.y, grid.z}, {block.x, block.y, block.z},
                        a.d.split_k, a.ktiles_per_split, a.tilesM, a.tilesN, a.cnt != nullptr};
    }
    return hipSuccess;
}
extern "C" hipError_t hipGetLastError(void) { return hipSuccess; }
extern "C" hipError_t hipGetSymbolAddress(void** p, const void*) { *p = g_counters; return hipSuccess; }
// the launches since the last call (at most 8), oldest first
extern "C" int shim_take(Rec* out) {
    const int n = g_n;
    for (int i = 0; i < n; ++i) out[i] = g_rec[i];
    g_n = 0;
    return n;
}
