// gmpi_band_masks.hpp -- the exec masks of the band kernel's DMA passes (render_band.hip `issue`), in closed form.
//
// A sub-block's box of `nq` items x `rows` texel rows is moved by the kSubLanes loader lanes of its waves in up to kNP passes.  Lane l of wave wj
// is loader lane t = 64 wj + l; its item of pass 0 sits in line t / kCols (line = 4 row + channel), item column t % kCols, texel row t / kIPR, and
// pass r moves the same item kRPP rows further down.  The lane takes part in pass r iff
//     t < kPassItems  &&  t % kCols < nq  &&  t / kIPR + r * kRPP < rows.
// Every input is wave-uniform, so the mask is a bit pattern of scalars -- mask = colmask(nq) & rowmask(rows - r kRPP):
//   rowmask: t / kIPR < n  <=>  t < kIPR n: a run of low bits, the lanes with t < kIPR min(n, kRPP);
//   colmask: the pattern (1 << nq) - 1 with period kCols, at phase (64 wj) % kCols in lane 0: the partial run that leads the wave by a shift,
//            the whole runs by ONE multiply with the wave's constant of run heads (ones where t % kCols == 0 and t < kPassItems -- the lane
//            limit is a whole number of runs, so it costs nothing).  nq <= kCols: the runs do not overlap, the product has no carries, and
//            what would land beyond lane 63 falls off the 64-bit product.
// A box needs passes 0 ... last = (rows - 1) / kRPP; the ones below `last` move whole passes of rows, i.e. their mask IS the column mask, and
// only pass `last` has a row limit of its own: passes() forms one column mask and one row run per box, whatever kNP.
// Plain C++ on uniform values: scalar instructions on the device (no lane index, no compare per lane, no ballot), and the same code on the host
// (tests/test_band_masks_cpu.py enumerates every case against the per-lane definition).
#pragma once

#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define GMPI_MASKS_HD __host__ __device__ __forceinline__
#else
#define GMPI_MASKS_HD inline
#endif

namespace gmpi {
namespace band {

template <int kCols, int kIPR, int kRPP, int kSubLanes, int kPassItems, int kNP>
struct LoaderMasks {
    static constexpr int kWaves = kSubLanes / 64;
    static_assert(kSubLanes % 64 == 0 && kWaves >= 1, "whole waves");
    static_assert(kCols >= 1 && kCols < 32, "the column pattern is built in 32 bits");
    static_assert(kIPR == 4 * kCols && kPassItems == kRPP * kIPR && kPassItems <= kSubLanes && kRPP >= 1 && kNP >= 1, "geometry");

    // item column of the wave's lane 0
    static constexpr int phase(int wj) { return (64 * wj) % kCols; }
    // ones in the lanes behind lane 0 that start a run (t % kCols == 0, t < kPassItems); the run of lane 0, whole or entered in its middle, is the "leading" one
    static constexpr uint64_t heads(int wj) {
        uint64_t h = 0;
        for (int l = kCols - phase(wj); l < 64 && 64 * wj + l < kPassItems; l += kCols) h |= uint64_t(1) << l;
        return h;
    }
    // the per-wave constants by a compare chain (wj is a run-time scalar; the chain folds to selects of literals, taken once per kernel)
    static GMPI_MASKS_HD uint64_t heads_of(int wj) {
        uint64_t h = heads(0);
        for (int w = 1; w < kWaves; ++w) h = wj == w ? heads(w) : h;
        return h;
    }
    static_assert(64 * (kWaves - 1) < kPassItems, "every wave holds loader lanes (its leading run lies below the lane limit)");
    static GMPI_MASKS_HD int phase_of(int wj) {
        int p = phase(0);
        for (int w = 1; w < kWaves; ++w) p = wj == w ? phase(w) : p;
        return p;
    }

    // lanes of wave wj below the lane limit whose item column is below nq (0 <= nq <= kCols)
    static GMPI_MASKS_HD uint64_t colmask(int nq, int wj) {
        const uint32_t run = (uint32_t(1) << nq) - 1u;
        const uint32_t lead = run >> phase_of(wj);   // columns phase ... kCols - 1 in lanes 0 ... (the whole run when the phase is 0)
        return lead | uint64_t(run) * heads_of(wj);
    }
    // the run of low bits: lanes of wave wj with t < lim (any int)
    static GMPI_MASKS_HD uint64_t lowrun(int lim, int wj) {
        const int over = 64 * (wj + 1) - lim;                // lanes of the wave at and above the limit
        const int sh = over < 0 ? 0 : over;                  // (written as shift, maximum and one select: a saturating form would be vector-only)
        return sh < 64 ? ~uint64_t(0) >> (sh & 63) : uint64_t(0);
    }
    // lanes of wave wj below the lane limit whose pass-0 texel row is below rows_left (any int: <= 0 gives no lane)
    static GMPI_MASKS_HD uint64_t rowmask(int rows_left, int wj) { return lowrun(kIPR * (rows_left < kRPP ? rows_left : kRPP), wj); }
    // the exec mask of pass r (0 <= r < kNP) for wave wj of a sub-block whose box has nq items per line and `rows` texel rows
    static GMPI_MASKS_HD uint64_t pass(int nq, int rows, int wj, int r) { return colmask(nq, wj) & rowmask(rows - r * kRPP, wj); }

    // All passes of a box (rows >= 0) from one column mask and one row run: pass r < last moves `cols`, pass `last` moves `part`, the passes behind it nothing.
    struct Passes {
        uint64_t cols, part;
        int last;
        GMPI_MASKS_HD uint64_t operator[](int r) const { return r < last ? cols : r == last ? part : uint64_t(0); }
    };
    // (the caller knows `last`: the kernel branches on the number of passes anyway, and with a literal `last` the row run is a handful of instructions)
    static GMPI_MASKS_HD Passes passes(int nq, int rows, int wj, int last) {
        Passes p;
        p.last = last;
        p.cols = colmask(nq, wj);
        p.part = p.cols & lowrun(kIPR * rows - last * kPassItems, wj);
        return p;
    }
    static GMPI_MASKS_HD Passes passes(int nq, int rows, int wj) { return passes(nq, rows, wj, (rows - 1) / kRPP); }   // (rows == 0: pass 0, with an empty row run)
};

}  // namespace band
}  // namespace gmpi
