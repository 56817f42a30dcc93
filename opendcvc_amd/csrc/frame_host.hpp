// frame_host.hpp - the host scaffolding every picture-side entry shares (host only: no device code).  The object is a model
// frame [3][Hp][Wp] of _Float16 or float whose top-left H x W is the picture (typed / with_flag, the dispatch on the storage
// type and on a compile-time switch, are common.hpp's):
//   check_frame         the argument check of one frame, one wording; an entry keeps only the checks that are its own
//   vec_ok              may a launch use accesses of `elems` elements
//   tile_grid           the grid of a launch with a workgroup per TW x TH tile of each of the three planes
#pragma once
#include <cstdint>

#include "common.hpp"

namespace dcvc {

// the frame `what` of entry `who`; no device is touched
inline int check_frame(const char* who, const char* what, int dtype, const void* p, int Hp, int Wp, int H, int W)
{
    DCVC_REQUIRE(dtype == DCVC_F16 || dtype == DCVC_F32, "%s: bad dtype %d", who, dtype);
    DCVC_REQUIRE(p, "%s: %s is a null pointer", who, what);
    DCVC_REQUIRE(H > 0 && W > 0, "%s: bad picture size %d x %d", who, H, W);
    DCVC_REQUIRE(Hp >= H && Wp >= W, "%s: %s (%d x %d) does not hold the picture (%d x %d)", who, what, Hp, Wp, H, W);
    DCVC_REQUIRE((uintptr_t)p % elem_size(dtype) == 0, "%s: %s is not aligned to its element size", who, what);
    DCVC_REQUIRE((int64_t)3 * Hp * Wp < ((int64_t)1 << 40), "%s: %s (%d x %d) is too large", who, what, Hp, Wp);
    return 0;
}

// every pointer is aligned to `elems` elements of `es` bytes and so is every row (Wp elements long)
template <typename... P>
bool vec_ok(int elems, size_t es, int64_t Wp, const P*... p)
{
    const uintptr_t bytes = (uintptr_t)elems * es;
    return (((uintptr_t)p % bytes == 0) && ...) && Wp % elems == 0;
}

// grid = tiles of TW columns x tiles of TH rows x 3 planes of an Hp x Wp frame
inline int tile_grid(const char* who, int Wp, int Hp, int TW, int TH, dim3& grid)
{
    grid = dim3((unsigned)((Wp + TW - 1) / TW), (unsigned)((Hp + TH - 1) / TH), 3);
    DCVC_REQUIRE(grid.y <= 65535u, "%s: height %d above %d", who, Hp, 65535 * TH);
    return 0;
}

}  // namespace dcvc
