// dcvc_deint_field.hip - the second picture of field-rate deinterlacing (docs/deinterlace.md, "Field-rate output"; numpy:
// tests/deint_field_ref.py).  B_n = D(S_n, S_{n-1}, 1 - p): the document's filter, unchanged, on the field-shifted frames
//   S_n      rows with (y / L) % 2 != p from F_n (its second field), the others from F_{n+1} (its first field)
//   S_{n-1}  rows with (y / L) % 2 != p from F_{n-1},                the others from F_n
// with the OTHER parity kept - so the rows of F_n's second field pass bit for bit and the rows between them are rebuilt at
// the half instant.  Neither S is ever made: the kernel is dcvc_deinterlace's own (deint_shared.hpp: deinterlace_kernel, one
// copy for both entries, here with FIELD set), and the ONE difference is the frame a staged row is read from, chosen by the
// parity of the (clamped) row in its plane: uniform over a row, a select on a pointer.  The traffic is cur whole, half of
// before, half of after and one frame written - dcvc_deinterlace's three frames.  With before or after NULL the picture is
// step 5, the spatial predictor alone, which reads the kept rows only: every row is staged from cur, no neighbour is touched.
#include "common.hpp"
#include "deint_shared.hpp"
#include "frame_host.hpp"
#include "plane_math.hpp"

#include <cstdint>

extern "C" int dcvc_deinterlace_field(int dtype, const void* before_nchw, const void* cur_nchw, const void* after_nchw, int Hp, int Wp,
                                      int H, int W, int keep_parity, int chroma_lines, void* out_nchw, void* stream)
{
    const char* who = "dcvc_deinterlace_field";
    if (int rc = dcvc::check_frame(who, "the current frame", dtype, cur_nchw, Hp, Wp, H, W)) return rc;
    if (before_nchw)
        if (int rc = dcvc::check_frame(who, "the frame before", dtype, before_nchw, Hp, Wp, H, W)) return rc;
    if (after_nchw)
        if (int rc = dcvc::check_frame(who, "the frame after", dtype, after_nchw, Hp, Wp, H, W)) return rc;
    if (int rc = dcvc::check_frame(who, "out", dtype, out_nchw, Hp, Wp, H, W)) return rc;
    DCVC_REQUIRE(keep_parity == 0 || keep_parity == 1, "%s: keep_parity %d is not 0 (top field) or 1 (bottom field)", who, keep_parity);
    DCVC_REQUIRE(chroma_lines == 1 || chroma_lines == 2, "%s: chroma_lines %d is not 1 or 2", who, chroma_lines);
    DCVC_REQUIRE(H % (2 * chroma_lines) == 0, "%s: height %d is not a multiple of %d (two fields of %d-row lines)", who, H,
                 2 * chroma_lines, chroma_lines);
    const size_t es = dcvc::elem_size(dtype);
    const uint64_t bytes = (uint64_t)3 * Hp * Wp * es;
    const auto overlaps = [&](const void* p) {
        return p && (uintptr_t)out_nchw < (uintptr_t)p + bytes && (uintptr_t)p < (uintptr_t)out_nchw + bytes;
    };
    DCVC_REQUIRE(!overlaps(cur_nchw), "%s: out overlaps the current frame (neighbours are read)", who);
    DCVC_REQUIRE(!overlaps(before_nchw), "%s: out overlaps the frame before (neighbours are read)", who);
    DCVC_REQUIRE(!overlaps(after_nchw), "%s: out overlaps the frame after (neighbours are read)", who);
    dim3 grid;
    if (int rc = dcvc::tile_grid(who, Wp, Hp, TW, TH, grid)) return rc;
    const bool both = before_nchw && after_nchw;             // else step 5: neither neighbour is read
    const bool vec = dcvc::vec_ok(16 / (int)es, es, Wp, cur_nchw, out_nchw) &&
                     (!both || dcvc::vec_ok(16 / (int)es, es, Wp, before_nchw, after_nchw));
    return dcvc::typed(dtype, [&](auto tag) {
        using T = decltype(tag);
        dcvc::with_flag(vec, [&](auto v) {
            dcvc::with_flag(both, [&](auto b) {
                // (the shifted frames keep the OTHER parity; the kernel's `prev` is S_(n-1)'s other source, the frame before)
                deinterlace_kernel<T, decltype(v)::value, decltype(b)::value, true><<<grid, DB, 0, (hipStream_t)stream>>>(
                    nullptr, (const T*)cur_nchw, (const T*)before_nchw, (const T*)after_nchw, Hp, Wp, H, W, 1 - keep_parity,
                    chroma_lines, (T*)out_nchw);
            });
        });
    });
}
