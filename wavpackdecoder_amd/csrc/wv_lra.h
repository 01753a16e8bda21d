// wv_lra.h -- loudness range and short-term loudness (wvg_batch_loudness_range): EBU Tech
// 3342's 3 s short-term power every 100 ms, its two gates and the 10th and 95th percentile
// of what passes them, over the step energies that wvg_batch_loudness leaves on the device.
//
// The step energies E[channel][step], the weights G_c and the LdFile table are loudness's
// (wv_loud.h).  Thirty steps and the channel weights make a short-term power ST_j, the gate
// code of wv_loud.h with the factor 0.01 makes the counts, the mean and the relative gate,
// and a radix select finds the two order statistics exactly.  The definition is in
// include/wvgpu.h; this header is its code.
//
// Three passes, no float atomics:
//   short:   one thread per ST_j of the short-term image.
//   gate:    one wave per file: ld_gate_part / ld_gate_merge over the file's ST_j, twice.
//   select:  one workgroup per file.  Every ST_j is >= +0.0 and finite, so the 64-bit
//            patterns of the doubles order as unsigned integers.  Eight passes of eight bits,
//            most significant first: a pass counts, per rank, the values that pass the gates
//            and share the rank's known high bytes into 256 bins by their next byte, walks
//            the bins to the one that holds the rank, appends its byte and lowers the rank by
//            the count of the bins before it.  Both ranks go through the same passes.  Counts
//            are integers, so no scheduling changes a result, and an order statistic of a
//            multiset does not depend on how it is found.
//
// The code is compiled for the host and the device (WVF_HD) with contraction off, as
// wv_loud.h: the kernels (wv_lra.hip) call it once per thread, the host entries
// wvg_loudness_range_ints / _gate with the thread index as a loop.  Every offset is 64-bit.
#pragma once
#include "wv_loud.h"

#if defined(__clang__)
#pragma clang fp contract(off)
#elif defined(__GNUC__)
#pragma GCC push_options
#pragma GCC optimize("fp-contract=off")
#endif

namespace wvg {

constexpr uint32_t kLrShortSteps = 30;      // steps of one short-term window (3 s)
constexpr uint32_t kLrShortThreads = 256;   // threads of one workgroup of the short kernel
constexpr uint32_t kLrSelectThreads = 256;  // threads of one workgroup of the select kernel
constexpr uint32_t kLrHeld = 4;             // values a select thread keeps in registers over the passes
constexpr uint32_t kLrBins = 256, kLrPasses = 8;
constexpr double kLrRelFactor = 0.01;       // the relative gate: -20 LU

// one per measurable file, beside its LdFile
struct LrFile {
    uint64_t st_off;   // the file's first ST_j in the short-term image
    uint32_t nshort;   // max(0, nsteps - 29)
    uint32_t pad;
};

// wvg_file_loudness_range (include/wvgpu.h), field for field
struct LrRecord {
    double low_power, high_power, max_short_power, ungated_short_power;
    int64_t shorts, abs_shorts, gated_shorts, short_offset;
};

WVF_HD uint32_t lr_nshort(uint32_t nsteps) { return nsteps >= kLrShortSteps ? nsteps - (kLrShortSteps - 1u) : 0u; }

// the file that holds value `idx` of the short-term image: the last file whose st_off is
// <= idx (ld_find_file's rule: files of no values share their successor's offset and come
// before it)
WVF_HD uint32_t lr_find_file(const LrFile *files, uint32_t nfiles, uint64_t idx) {
    uint32_t lo = 0, hi = nfiles;
    while (hi - lo > 1u) {
        const uint32_t mid = lo + (hi - lo) / 2u;
        if (files[mid].st_off <= idx) lo = mid;
        else hi = mid;
    }
    return lo;
}

// ST_j of a file: channels ascending, each channel's thirty steps ascending
WVF_HD double lr_short(const LdFile &f, const double *E, const double *w, uint32_t j) {
    double acc = 0.0;
    for (uint32_t c = 0; c < f.nch; c++) {
        const double *e = E + (uint64_t)c * f.nsteps + j;
        double t = e[0];
        WV_LD_UNROLL
        for (uint32_t i = 1; i < kLrShortSteps; i++) t = t + e[i];
        acc = ld_fma(w[c], t, acc);
    }
    return acc / (double)(kLrShortSteps * (uint64_t)f.S);
}

// ---- gate ----
WVF_HD double lr_rel(const LdGate &ungated) { return kLrRelFactor * ld_gate_mean(ungated); }

// the gate's part of the record; the select pass fills low_power and high_power
WVF_HD void lr_record(const LrFile *f, uint64_t n, const LdGate &ungated, const LdGate &gated, LrRecord *out) {
    LrRecord r;
    r.low_power = r.high_power = 0.0;
    r.max_short_power = ungated.mx;
    r.ungated_short_power = ld_gate_mean(ungated);
    r.shorts = (int64_t)n;
    r.abs_shorts = ungated.cnt;
    r.gated_shorts = gated.cnt;
    r.short_offset = f ? (int64_t)f->st_off : 0;
    *out = r;
}

// ---- select ----
WVF_HD bool lr_gated(double v, double rel) { return v > kLdAbsGate && v > rel; }

WVF_HD uint64_t lr_bits(double v) {
    uint64_t u;
    memcpy(&u, &v, 8);
    return u;
}

WVF_HD double lr_value(uint64_t u) {
    double v;
    memcpy(&v, &u, 8);
    return v;
}

// libebur128's percentile indices into the n sorted values (n >= 1), in integers
WVF_HD uint64_t lr_low_rank(uint64_t n) { return (n + 4u) / 10u; }
WVF_HD uint64_t lr_high_rank(uint64_t n) { return (19u * (n - 1u) + 10u) / 20u; }

// a rank on its way down the eight passes: the high bytes found so far and the rank among
// the values that share them
struct LrRank {
    uint64_t prefix, rank;
};

WVF_HD uint32_t lr_shift(uint32_t pass) { return 56u - 8u * pass; }

// the bytes of a pattern that the passes before `pass` have decided
WVF_HD uint64_t lr_known(uint64_t u, uint32_t pass) { return pass ? u & (~0ull << (64u - 8u * pass)) : 0ull; }

WVF_HD uint32_t lr_digit(uint64_t u, uint32_t pass) { return (uint32_t)(u >> lr_shift(pass)) & (kLrBins - 1u); }

// whether pattern `u` is still a candidate of `r` in `pass`
WVF_HD bool lr_candidate(uint64_t u, const LrRank &r, uint32_t pass) { return lr_known(u, pass) == r.prefix; }

// The histogram walk, by the 64 lanes of one wave: lane l owns the kLrWalkBins bins from
// l * kLrWalkBins on.  lr_walk_sum is what a lane's bins hold (a file has fewer than 2^31
// values, so 32 bits do); the sums before a lane's -- an exclusive prefix over the lanes, a
// scan on the device, a running sum on the host -- tell it whether the rank lies in its bins.
// The one lane where it does appends the bin's byte to the prefix and lowers the rank by
// what the bins before that bin hold.
constexpr uint32_t kLrWalkLanes = 64, kLrWalkBins = kLrBins / kLrWalkLanes;

WVF_HD uint32_t lr_walk_sum(const uint32_t *hist, uint32_t lane) {
    uint32_t s = 0;
    for (uint32_t i = 0; i < kLrWalkBins; i++) s += hist[lane * kLrWalkBins + i];
    return s;
}

// `before`: the sum of the lanes before this one.  True for the lane that holds the rank.
WVF_HD bool lr_walk_lane(const uint32_t *hist, uint32_t lane, uint64_t before, LrRank &r, uint32_t pass) {
    uint64_t cum = before;
    for (uint32_t i = 0; i < kLrWalkBins; i++) {
        const uint32_t bin = lane * kLrWalkBins + i;
        const uint64_t h = hist[bin];
        if (r.rank >= cum && r.rank < cum + h) {
            r.prefix |= (uint64_t)bin << lr_shift(pass);
            r.rank -= cum;
            return true;
        }
        cum += h;
    }
    return false;
}

}  // namespace wvg

#if !defined(__clang__) && defined(__GNUC__)
#pragma GCC pop_options
#endif
