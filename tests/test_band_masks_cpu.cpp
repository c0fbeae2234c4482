// Host check of ml-gmpi_amd/csrc/gmpi_band_masks.hpp (built and run by test_band_masks_cpu.py): every (items, rows, wave, pass) of every loader
// geometry render_band.hip's Geo can take, against the per-lane definition the masks used to be balloted from.
#include <cstdint>
#include <cstdio>

#include "gmpi_band_masks.hpp"

// Geo<TexT> of render_band.hip for an element size and a pixels-per-thread build parameter (GMPI_BAND_PPT16 / GMPI_BAND_PPT32)
template <int ES, int PPT> struct Geo {
    static constexpr int SBH = 8, WPS = SBH / PPT, kSubLanes = 64 * WPS;
    static constexpr int kCols = ES == 2 ? 10 : 20, kIPR = 4 * kCols, kMaxRows = 15;
    static constexpr int kRPP = kSubLanes / kIPR, kPassItems = kRPP * kIPR, kNP = (kMaxRows + kRPP - 1) / kRPP;
    static_assert(kNP == 3 || kNP == 5, "passes");
    using Masks = gmpi::band::LoaderMasks<kCols, kIPR, kRPP, kSubLanes, kPassItems, kNP>;
};

template <typename G> static long check(const char* name, long want_cases, int& failures) {
    long cases = 0;
    for (int nq = 0; nq <= G::kCols; ++nq)
        for (int rows = 0; rows <= G::kMaxRows; ++rows)
            for (int wj = 0; wj < G::WPS; ++wj)
                for (int r = 0; r < G::kNP; ++r, ++cases) {
                    uint64_t want = 0;
                    for (int l = 0; l < 64; ++l) {
                        const int t = 64 * wj + l;
                        if (t < G::kPassItems && (t % G::kCols) < nq && (t / G::kIPR) + r * G::kRPP < rows) want |= uint64_t(1) << l;
                    }
                    const uint64_t got = G::Masks::pass(nq, rows, wj, r);
                    const uint64_t split = G::Masks::colmask(nq, wj) & G::Masks::rowmask(rows - r * G::kRPP, wj);
                    // the padded boxes' masks: every item column of the box rows
                    uint64_t want_rows = 0;
                    for (int l = 0; l < 64; ++l) {
                        const int t = 64 * wj + l;
                        if (t < G::kPassItems && (t / G::kIPR) + r * G::kRPP < rows) want_rows |= uint64_t(1) << l;
                    }
                    const uint64_t got_rows = G::Masks::rowmask(rows - r * G::kRPP, wj);
                    // the form the kernel issues from: one column mask and one row run per box
                    const typename G::Masks::Passes p = G::Masks::passes(nq, rows, wj);
                    const uint64_t by_box = p[r];
                    const int want_last = rows > 0 ? (rows - 1) / G::kRPP : 0;
                    if (got != want || split != want || got_rows != want_rows || by_box != want || p.last != want_last) {
                        if (failures++ < 10)
                            std::printf("%s: nq %d rows %d wave %d pass %d: mask %016llx, per box %016llx (last pass %d), definition %016llx; row mask %016llx, definition %016llx\n",
                                        name, nq, rows, wj, r, (unsigned long long)got, (unsigned long long)by_box, p.last, (unsigned long long)want,
                                        (unsigned long long)got_rows, (unsigned long long)want_rows);
                    }
                }
    std::printf("%s: %ld cases (cols %d, rows per pass %d, lanes %d, passes %d)\n", name, cases, G::kCols, G::kRPP, G::kSubLanes, G::kNP);
    if (want_cases > 0 && cases != want_cases) {
        std::printf("%s: expected %ld cases\n", name, want_cases);
        ++failures;
    }
    return cases;
}

int main() {
    int failures = 0;
    check<Geo<2, 2>>("16-bit, 2 pixels per thread (as shipped)", 11L * 16 * 4 * 3, failures);
    check<Geo<4, 2>>("fp32, 2 pixels per thread (as shipped)", 21L * 16 * 4 * 5, failures);
    check<Geo<2, 4>>("16-bit, 4 pixels per thread", 11L * 16 * 2 * 5, failures);
    check<Geo<4, 1>>("fp32, 1 pixel per thread", 21L * 16 * 8 * 3, failures);
    if (failures) std::printf("FAILED: %d\n", failures);
    else std::printf("ok\n");
    return failures ? 1 : 0;
}
