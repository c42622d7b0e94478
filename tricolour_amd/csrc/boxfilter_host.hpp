// Host side of the box-filter family (kernels_boxfilter / boxline / boxpipe / boxweight / boxexact.hpp), included by
// tricolour_amd.hip inside its host namespace: the pure picks -- functions of (BoxRoutes, shape, alignment) that name a
// kernel instantiation completely -- and the launchers, launch_x(run, pick, job), which only switch on a pick.
// "Which instantiation does shape X take under switch Y" is answered by pick_col_filter() and pick_freq_stage().

// ---- integer -> template argument ----------------------------------------------------------------------------------
// with_constant(v, Ints<...>{}, none, f) calls f(std::integral_constant<int, K>) for the K that equals v and returns what it
// returns (a TRI_* code); when the list does not hold v there is no such instantiation: TRI_EINVAL with the message `none`
// (one %d: v).  The lists below ARE the instantiated sets: the picks test membership with one_of(), the launchers dispatch
// over the same list.
template <int... Ks> using Ints = std::integer_sequence<int, Ks...>;
template <int... Ks, class F>
static int with_constant(int v, Ints<Ks...>, const char* none, F&& f) {
    int rc = TRI_OK;
    const bool hit = ((v == Ks && ((rc = f(std::integral_constant<int, Ks>{})), true)) || ...);
    return hit ? rc : set_err(TRI_EINVAL, none, v);
}
template <int... Ks>
static constexpr bool one_of(int v, Ints<Ks...>) { return ((v == Ks) || ...); }
// the first K of the list that `accept` takes, or 0
template <int... Ks, class P>
static int first_of(Ints<Ks...>, P&& accept) {
    int out = 0;
    (void)((accept(Ks) && ((out = Ks), true)) || ...);
    return out;
}
template <int FIRST, int STEP, int... I>
static constexpr auto int_range(Ints<I...>) { return Ints<FIRST + STEP * I...>{}; }

// ---- radius limits and compile-time knobs --------------------------------------------------------------------------
// Radius limits of the single-sweep kernels.  r <= LDS_R_MAX: K4b with 256
// threads (4 rings per thread); r <= LANE4_R_MAX: K4c (one ring per thread);
// beyond: the in-place multi-pass kernel.
// Measured crossovers (scripts/build_variants.sh -DLDS_R_MAX=.. -DLANE4_R_MAX=..): four rings per thread win
// up to r = 15 (256 threads to r = 10, 128 beyond; K4c needs 2r >= 32 anyway), one ring per thread up to
// r = 160 (two waves per CU), the multi-pass kernel beyond.
#ifndef LDS_R_MAX
#define LDS_R_MAX 15
#endif
#ifndef LANE4_R_MAX
#define LANE4_R_MAX 160
#endif
// LDS budget of the single-sweep filter: 4 stages x 2r slots x BT threads x 4 B.  Returns the block size to use, or 0 when
// the radius is too large and the in-place multi-pass kernel must be used instead.
static int narrowed(int bt, int C) {      // (no wider than the columns need)
    while (bt > 64 && bt / 2 >= C) bt /= 2;
    return bt;
}
static int colfilter_lds_block(const BoxRoutes& b, int rad, int C) {
    if (b.multipass || rad <= 0) return 0;
    if (!b.lane4) return narrowed(rad <= 10 ? 256 : (rad <= 20 ? 128 : (rad <= 40 ? 64 : 0)), C);   // K4b alone (TRI_FILTER_NO_LANE4)
    if (rad <= LDS_R_MAX) return narrowed(rad <= 10 ? 256 : 128, C);
    return rad <= LANE4_R_MAX ? 64 : 0;
}
static bool colfilter_use_lane4(const BoxRoutes& b, int rad) { return b.lane4 && rad > LDS_R_MAX && rad <= LANE4_R_MAX; }

// Register-ring single sweep (K4r, kernels_boxline.hpp): KS register slots per stage, the
// rest of the 2r-deep delay line in LDS.  Returns 0 when the radius is outside its range.
#ifndef BOXR_MAX_LDS_SLOTS
#define BOXR_MAX_LDS_SLOTS 60
#endif
static int boxr_pick_ks(const BoxRoutes& b, int rad) {
    if (!b.reg_rings || rad < 4 || rad > 107) return 0;
    const int ks = 2 * rad >= 80 ? 80 : (2 * rad >= 64 ? 64 : (2 * rad >= 32 ? 32 : (2 * rad >= 16 ? 16 : 8)));
    return 2 * rad - ks <= BOXR_MAX_LDS_SLOTS ? ks : 0;
}
// the time-axis stage keeps K4b below 16 slots (already at the HBM floor there); the fused
// frequency stage takes the register form from r = 4 on
#ifndef BOXT_MIN_2R
#define BOXT_MIN_2R 32
#endif
#ifndef BOXT_EXACT20
#define BOXT_EXACT20 1                   // r = 10: all 20 slots of a delay line in registers (k_boxt<20, false, *>): no LDS traffic at all,
                                         // 11.7 ms per 1008-window launch pair against 13.9 for the LDS delay lines (K4b)
#endif
static int boxr_pick_ks_t(const BoxRoutes& b, int rad) {
    if (BOXT_EXACT20 && 2 * rad == 20) return boxr_pick_ks(b, rad) > 0 ? 20 : 0;
    return 2 * rad >= BOXT_MIN_2R ? boxr_pick_ks(b, rad) : 0;
}
static int boxr_pick_ks_f(const BoxRoutes& b, int rad) { return b.reg_rings_f ? boxr_pick_ks(b, rad) : 0; }

// K4w (kernels_boxweight.hpp): the weight image of the time-axis stage in integer arithmetic, one thread per line, for
// 20 <= 2r <= 110 -- every radius the register-delay-line kernels (K4r, K4q) serve on that axis.  False: the family's own
// kernel filters the weight image as well.
using BoxwRadii = decltype(int_range<10, 1>(std::make_integer_sequence<int, 46>{}));                  // k_boxw<2r>, r = 10 .. 55
static bool boxw_usable(const BoxRoutes& b, int rad, int n, int C) {
    return b.boxw && 2 * rad >= 20 && 2 * rad <= 110 && n % 4 == 0 && (uint64_t)n * (uint64_t)C * 4u < (1ull << 31);
}

// Stage-pipelined spectrum filter (K4p, kernels_boxpipe.hpp): block length B for radius rad, 0 when it does not apply
// (2r >= B, four stage buffers within the CU's 160 KB of LDS).
static int boxp_pick_block(const BoxRoutes& b, int rad, int C) {
    if (b.spec_pipe == SpecPipe::Off) return 0;
    if (b.spec_pipe != SpecPipe::B8 && 2 * rad >= 16 && C % 4 == 0 && boxp_lds_bytes(rad, 16) <= 160 * 1024) return 16;
    if (b.spec_pipe == SpecPipe::B16) return 0;
    if (2 * rad >= 8 && C % 2 == 0 && boxp_lds_bytes(rad, 8) <= 160 * 1024) return 8;
    return 0;
}

// K4q / K4qf (kernels_boxpipe.hpp): register part of the delay lines with blocks of 16 positions, 0 when there is none
using BoxqKs16 = Ints<16, 32, 48, 64, 80, 96>;         // k_boxq<KS, ., 16>, k_boxqf<KS, ., 16>
static int boxq_pick_ks(int rad) { return one_of(2 * rad / 16 * 16, BoxqKs16{}) ? 2 * rad / 16 * 16 : 0; }
#ifndef BOXQ_MIN_2R
#define BOXQ_MIN_2R 56
#endif
// blocks of 8 positions (four workgroups = four waves per SIMD) while the delay line fits 128 registers: KS = 8 * floor(2r / 8)
#ifndef BOXQ_B8_MIN_2R
#define BOXQ_B8_MIN_2R 32
#endif
#ifndef BOXQ_B8_MAX2R
#define BOXQ_B8_MAX2R 88
#endif
// (72: the data image's kernel would spill 7 registers at 128 -- blocks of 16 with KS = 64 take 2r = 72 .. 78)
using BoxqKs8 = Ints<32, 40, 48, 56, 64, 80>;          // k_boxq<KS, ., 8>
static int boxq_pick_ks8(const BoxRoutes& b, int rad) {
    return (b.pipe_t_b8 && 2 * rad >= BOXQ_B8_MIN_2R && 2 * rad < BOXQ_B8_MAX2R) ? 2 * rad / 8 * 8 : 0;
}
// blocks of 8 with FIFOs one block deeper (k_boxq_deep): KS = 80 for 2r = 88 .. 95, KS = 96 for 2r = 104 .. 111
#ifndef BOXQ_DEEP
#define BOXQ_DEEP 1
#endif
using BoxqDeepKs = Ints<80, 96>;

// K4qf: the fused frequency stage as an eight-wave stage pipeline (kernels_boxpipe.hpp)
#ifndef BOXQF_MIN_2R
#define BOXQF_MIN_2R 34
#endif
#ifndef BOXQF_FEW_WAVES
#define BOXQF_FEW_WAVES 2048             // waves a K4r launch needs to fill the machine at two per SIMD
#endif
#ifndef BOXQF_B8_MAX2R
#define BOXQF_B8_MAX2R 88                // blocks of 8 positions below this delay (56: up to 48 registers; 72: up to 64; 88: up to 80)
#endif
// k_boxqf<KS, ., 8>: up to 48 slots always, up to 64 / 80 / 96 as the knob allows; of 80 only MODE 1 (MODE 2 would spill 11
// registers at 128: blocks of 16 for it)
using BoxqfKs8 = Ints<16, 24, 32, 40, 48, 56, 64, 72, 80, 96>;
static constexpr bool boxqf_b8_exists(int ks, int mode) {
    constexpr int M = BOXQF_B8_MAX2R;
    return one_of(ks, BoxqfKs8{}) && (ks <= 48 || (ks <= 64 && M > 56) || (ks <= 80 && M > 72) || M > 88) && !(ks == 80 && mode == 2);
}

using BoxtKs = Ints<16, 20, 32, 64, 80>;               // k_boxt
using BoxtSpecKs = Ints<8, 16, 32, 64, 80>;            // k_boxt_spec
using BoxfKs = Ints<8, 16, 32, 64, 80>;                // k_boxf

// K4x: the frequency-axis stage + masked division for any radius, one line pair resident in LDS, lanes =
// positions, exactness checked per pass with a sequential redo (kernels_boxexact.hpp).  Rows in, rows out.
// The flagger takes it where no stage pipeline exists (r >= 56: final_st_very_broad's 277 / 221 / 166 / 110).
#ifndef BOXX_MIN_R
#define BOXX_MIN_R 56
#endif
// threads per image (128 or 256, << 8) | chunk length: the k_boxx<NTI, L, ., .> that exist, in the order they are tried
using BoxxCodes = Ints<128 << 8 | 37, 128 << 8 | 41, 256 << 8 | 17, 256 << 8 | 19, 256 << 8 | 21, 256 << 8 | 25>;
// The code of the instantiation for a line of n positions, or 0.  Long chunks on 128 threads per image where the line fits
// them (fewer instructions per line: see the kernel); BoxRoutes::exact_nti = 256 forces the short chunks (A/B runs).
static int boxx_pick_l(const BoxRoutes& b, int rad, int n) {
    if (b.exact == Want::Off || (b.exact == Want::Auto && rad < BOXX_MIN_R)) return 0;
    if (rad < 1 || n % 4 != 0) return 0;
    const int64_t P = (int64_t)n + 4 * (int64_t)rad;
    return first_of(BoxxCodes{}, [&](int c) {
        const int nti = c >> 8, l = c & 255;
        if (b.exact_nti && nti != b.exact_nti) return false;
        if (nti == 128 && (P <= 128 * 17 || rad < 64)) return false;      // (short lines / small radii: the short chunks do)
        if ((int64_t)nti * l < P || l > 2 * rad + 1 || (2 * rad + 1) / l > BOXX_AMAX) return false;
        return boxx_lds_bytes(nti, l, rad) <= 159 * 1024;
    });
}
// the reciprocal division is verified exhaustively for these radii only (test_division_by_box_denominator)
static bool boxx_recip_ok(int rad) { return rad <= 128 || rad == 166 || rad == 221 || rad == 277 || rad == 397 || rad == 795; }

// ---- time-axis stage and spectra: pick ------------------------------------------------------------------------------
// Where launch_colfilter() takes the two images from
enum class ColSrc {
    ByteFlags,     // built on the fly from (srcData, srcFlags) [n][C], one flag byte per sample
    Images,        // float arrays: for the multi-pass kernel in rows [4r, 4r+n) of bufW / bufO, for the LDS kernels in rows [0,n)
    PackedFlags    // built on the fly from (srcData, srcFlags), four line positions of a column per flag word (n % 4 == 0)
};
// COL_TRANSPOSED_OUT: write [C][n] (LDS-ring kernel, float images only); COL_WEIGHTS_01: the weights are 0 / 1 (integer arithmetic where exact)
enum ColFlag : unsigned { COL_TRANSPOSED_OUT = 1, COL_WEIGHTS_01 = 2 };
// K4p, K4r (spectrum), K4q, K4r, K4c, K4b, K4; MultiPassUnpadded: K4 on images without its n + 4r rows -- refused at the launch
enum class ColFamily { SpecPipe, SpecRing, StagePipe, RegRing, Lane4, LdsRing, MultiPass, MultiPassUnpadded };

// One axis of masked_gaussian_filter's two box filters (weight image and data image) on a column-layout image pair: the
// kernel instantiation(s) of one launch_colfilter()
struct ColPick {
    ColFamily fam = ColFamily::MultiPass;
    ColSrc src = ColSrc::Images;
    int ks = 0;               // SpecRing / RegRing / StagePipe: register slots per delay line
    int B = 0;                // SpecPipe / StagePipe: block length
    bool deep = false;        // StagePipe: k_boxq_deep
    int bt = 0;               // LdsRing: threads per block
    bool boxw = false, side = false;   // StagePipe / RegRing: the weight image through K4w; ... which goes to the run's side lane
    bool defers = false;      // the division by float32(d)**4 is left to the consumer (transpose / masked_div)
    bool transposed = false, intw = false;   // LdsRing: writes [C][n]; integer arithmetic for the weight image (exact while (2r+1)^4 <= 2^24)
};

// may_defer: the consumer can divide; spec_aligned: data / both outputs 16-byte and flags 4-byte aligned (K4p)
static ColPick pick_col_filter(const BoxRoutes& b, ColSrc src, unsigned flags, bool may_defer, int rad, int n, int C, int64_t W,
                               bool spec_aligned) {
    ColPick k;
    k.src = src;
    k.transposed = flags & COL_TRANSPOSED_OUT;
    const bool weights_are_01 = flags & COL_WEIGHTS_01;
    k.intw = weights_are_01 && rad <= 31;
    k.bt = colfilter_lds_block(b, rad, C);
    // the register-ring and stage-pipeline kernels build 0 / 1 weights themselves, divide themselves, write [n][C] and address
    // a window through signed 32-bit buffer offsets
    const bool regs_ok = !may_defer && !k.transposed && weights_are_01 && (uint64_t)n * (uint64_t)C * 4u < (1ull << 31);
    const bool spectrum = regs_ok && src == ColSrc::ByteFlags && W == 1;    // one "window" of byte flags + data, both images per launch
    const bool packed = regs_ok && src == ColSrc::PackedFlags && n % 4 == 0;
    if (spectrum && boxp_pick_block(b, rad, C) > 0 && rad <= 107 && spec_aligned) {
        k.fam = ColFamily::SpecPipe; k.B = boxp_pick_block(b, rad, C);
    } else if (spectrum && boxr_pick_ks(b, rad) > 0) {                      // from r = 4 on
        k.fam = ColFamily::SpecRing; k.ks = boxr_pick_ks(b, rad);
    }
    // measured (1008 windows, both images): K4r 13.4 / 13.5 / 14.6 / 15.9 / 19.2 / 21.9 / 19.9 / 23.0 / 23.7 ms at
    // r = 17 / 21 / 27 / 28 / 32 / 35 / 40 / 43 / 54; K4q with blocks of 8 (four waves per SIMD, r <= 43)
    // 15.3 / 15.8 / 16.0 / 15.9 / 16.1 / 16.3 / 17.2 / 17.3, with blocks of 16 19.3 ... 20.8
    else if (packed && b.pipe_t != Want::Off && boxq_pick_ks(rad) > 0 && rad <= 107 && (b.pipe_t == Want::Forced || 2 * rad >= BOXQ_MIN_2R)) {
        k.fam = ColFamily::StagePipe;
        const bool deep_on = BOXQ_DEEP && boxq_pick_ks8(b, 40) > 0;        // (blocks of 8 not switched off)
        if (deep_on && ((2 * rad >= 88 && 2 * rad < 96) || (2 * rad >= 104 && 2 * rad < 112))) {
            k.deep = true; k.B = 8; k.ks = 2 * rad < 96 ? 80 : 96;
        } else if (one_of(boxq_pick_ks8(b, rad), BoxqKs8{})) {
            k.B = 8; k.ks = boxq_pick_ks8(b, rad);
        } else {
            k.B = 16; k.ks = boxq_pick_ks(rad);
        }
    } else if (packed && boxr_pick_ks_t(b, rad) > 0) {
        k.fam = ColFamily::RegRing; k.ks = boxr_pick_ks_t(b, rad);
    } else if (k.bt > 0 && colfilter_use_lane4(b, rad) && !k.transposed && src != ColSrc::ByteFlags) {
        k.fam = ColFamily::Lane4; k.defers = may_defer;
    } else {
        if (k.bt > 0 && colfilter_use_lane4(b, rad) && src == ColSrc::ByteFlags) {
            // byte flags with a medium radius (no lane-per-stage kernel for them): 4-ring kernel with a small block if it fits
            k.bt = rad <= 20 ? 128 : (rad <= 40 ? 64 : 0);
            k.bt = narrowed(k.bt, C);
        }
        k.fam = k.bt > 0 ? ColFamily::LdsRing : (b.unpadded ? ColFamily::MultiPassUnpadded : ColFamily::MultiPass);
        // (the division is deferred for float images and packed flags only, the transposed output exists for float images only)
        k.defers = k.bt > 0 && may_defer && (src == ColSrc::PackedFlags || (src == ColSrc::Images && !k.transposed));
    }
    if (k.fam == ColFamily::StagePipe || k.fam == ColFamily::RegRing) {
        k.boxw = boxw_usable(b, rad, n, C);
        k.side = k.boxw && OVERLAP_TIME_STAGE >= (k.fam == ColFamily::RegRing ? 2 : 1);
    }
    return k;
}

// ---- time-axis stage and spectra: launch ----------------------------------------------------------------------------
// One sweep along the lines of W image pairs: n positions, C lines per window.  Output: rows [0,n) of dstW / dstO.
// bws / sws / dws: window strides of the buffers, the source and the destination.  Kernels that build their images from
// (srcData, srcFlags) ignore bufW / bufO.
struct ColJob {
    const float* srcData = nullptr; const uint8_t* srcFlags = nullptr;
    float *bufW = nullptr, *bufO = nullptr, *dstW = nullptr, *dstO = nullptr;
    int n = 0, C = 0, rad = 0;
    size_t bws = 0, sws = 0, dws = 0;
    int64_t W = 1;
};
// pick_col_filter()'s spec_aligned for a job
static bool spectrum_aligned(const ColJob& j) {
    return ((uintptr_t)j.srcData % 16 == 0) && ((uintptr_t)j.srcFlags % 4 == 0) && ((uintptr_t)j.dstW % 16 == 0) && ((uintptr_t)j.dstO % 16 == 0);
}

static int launch_boxw(const Run& r, const ColJob& j) {
    return with_constant(j.rad, BoxwRadii{}, "no integer weight filter for radius %d", [&](auto R) {
        hipLaunchKernelGGL((k_boxw<2 * R()>), dim3((unsigned)cdiv(j.C, 64), (unsigned)j.W), dim3(64), 0, r.st, j.srcFlags, j.dstW, j.n, j.C,
                           box_reciprocal(box_denominator(j.rad)), j.sws, j.dws);
        LAUNCHCHK();
        return (int)TRI_OK;
    });
}
// The two images of a family that filters one image per launch: image(std::integral_constant<int, I>) launches the kernel
// of the weight image (I = 0) or of the data image (I = 1) on r.st.  k.boxw: the weight image through K4w instead, beside the
// kernel of the data image -- they read the same flag words and write disjoint images.  k.side: K4w goes to the side lane of
// r, if it has one; both are done when r.st goes on.
template <class LaunchImage>
static int launch_both_images(const Run& r, const ColPick& k, const ColJob& j, LaunchImage&& image) {
    if (k.boxw) {
        const Run side = k.side ? fork(r) : r;
        const int rc = launch_boxw(side, j);
        if (!rc) image(std::integral_constant<int, 1>{});
        if (k.side) join(r);
        if (rc) return rc;
    } else {
        image(std::integral_constant<int, 0>{});
        image(std::integral_constant<int, 1>{});
    }
    LAUNCHCHK();
    return TRI_OK;
}

// K4r on the time axis: one launch per image -- a compute unit then runs (mostly) one of the two long loop bodies at a time
template <int KS>
static int launch_boxt_ks(const Run& r, const ColPick& k, const ColJob& j) {
    const int d = 2 * j.rad - KS;
    const size_t lds = (size_t)4 * d * 64 * sizeof(float);
    const float denom = box_denominator(j.rad);
    dim3 grid((unsigned)cdiv(j.C, 64), (unsigned)j.W);
    HIPCHK(lds_optin_all(160 * 1024, &k_boxt<KS, true, 0>, &k_boxt<KS, true, 1>));
    return launch_both_images(r, k, j, [&](auto I) {
        float* const dst = I() ? j.dstO : j.dstW;
        if (d > 0) hipLaunchKernelGGL((k_boxt<KS, true, I()>), grid, dim3(64), lds, r.st, j.srcData, j.srcFlags, dst, j.n, j.C, j.rad, denom, j.sws, j.dws);
        else hipLaunchKernelGGL((k_boxt<KS, false, I()>), grid, dim3(64), 0, r.st, j.srcData, j.srcFlags, dst, j.n, j.C, j.rad, denom, j.sws, j.dws);
    });
}
// K4q: blocks of B positions; DEEP: blocks of 8 with FIFOs one block deeper
template <int KS, int B, bool DEEP>
static int launch_boxq_ks(const Run& r, const ColPick& k, const ColJob& j) {
    dim3 grid((unsigned)cdiv(j.C, 64), (unsigned)j.W);
    const BoxDenom dn = box_reciprocal(box_denominator(j.rad));
    const auto kern = [](auto I) {
        if constexpr (DEEP) return &k_boxq_deep<KS, I()>;
        else return &k_boxq<KS, I(), B>;
    };
    const size_t lds = DEEP ? boxq_lds_bytes(8, 4) : boxq_lds_bytes(B);
    HIPCHK(lds_optin_all(160 * 1024, kern(std::integral_constant<int, 0>{}), kern(std::integral_constant<int, 1>{})));
    return launch_both_images(r, k, j, [&](auto I) {
        hipLaunchKernelGGL(kern(I), grid, dim3(256), lds, r.st, j.srcData, j.srcFlags, I() ? j.dstO : j.dstW, j.n, j.C, j.rad, dn, j.sws, j.dws);
    });
}
// Spectrum path (byte flags [n][C], a single "window", both images in one launch): K4r and K4p
template <int KS>
static int launch_boxt_spec_ks(const Run& r, const ColJob& j) {
    const int d = 2 * j.rad - KS;
    const size_t lds = (size_t)4 * d * 64 * sizeof(float);
    const float denom = box_denominator(j.rad);
    dim3 grid((unsigned)cdiv(j.C, 64), 2);
    HIPCHK(lds_optin_all(160 * 1024, &k_boxt_spec<KS, true>));
    if (d > 0) hipLaunchKernelGGL((k_boxt_spec<KS, true>), grid, dim3(64), lds, r.st, j.srcData, j.srcFlags, j.dstW, j.dstO, j.n, j.C, j.rad, denom);
    else hipLaunchKernelGGL((k_boxt_spec<KS, false>), grid, dim3(64), 0, r.st, j.srcData, j.srcFlags, j.dstW, j.dstO, j.n, j.C, j.rad, denom);
    LAUNCHCHK();
    return TRI_OK;
}
template <int B>
static int launch_boxp_spec_b(const Run& r, const ColJob& j) {
    HIPCHK(lds_optin_all(160 * 1024, &k_boxp_spec<B, 16>));
    dim3 grid((unsigned)cdiv(j.C, 64), 2);
    hipLaunchKernelGGL((k_boxp_spec<B, 16>), grid, dim3(256), boxp_lds_bytes(j.rad, B), r.st, j.srcData, j.srcFlags, j.dstW, j.dstO, j.n, j.C,
                       j.rad, box_denominator(j.rad));
    LAUNCHCHK();
    return TRI_OK;
}

static int launch_colfilter(const Run& r, const ColPick& k, const ColJob& j) {
    const int n = j.n, C = j.C, rad = j.rad;
    const float denom = box_denominator(rad);
    const bool built = k.src != ColSrc::Images, divide = !k.defers;
    const float *const inW = built ? nullptr : j.bufW, *const inO = built ? nullptr : j.bufO;
    const size_t in_ws = built ? 0 : j.bws;
    const char *const no_ring = "no register-ring kernel for %d slots", *const no_pipe = "no stage-pipeline kernel for %d slots";
    switch (k.fam) {
        case ColFamily::SpecPipe:
            return k.B == 16 ? launch_boxp_spec_b<16>(r, j) : launch_boxp_spec_b<8>(r, j);
        case ColFamily::SpecRing:
            return with_constant(k.ks, BoxtSpecKs{}, no_ring, [&](auto KS) { return launch_boxt_spec_ks<KS()>(r, j); });
        case ColFamily::StagePipe:
            if (k.deep) return with_constant(k.ks, BoxqDeepKs{}, no_pipe, [&](auto KS) { return launch_boxq_ks<KS(), 8, true>(r, k, j); });
            if (k.B == 8) return with_constant(k.ks, BoxqKs8{}, no_pipe, [&](auto KS) { return launch_boxq_ks<KS(), 8, false>(r, k, j); });
            return with_constant(k.ks, BoxqKs16{}, no_pipe, [&](auto KS) { return launch_boxq_ks<KS(), 16, false>(r, k, j); });
        case ColFamily::RegRing:
            return with_constant(k.ks, BoxtKs{}, no_ring, [&](auto KS) { return launch_boxt_ks<KS()>(r, k, j); });
        case ColFamily::Lane4: {
            HIPCHK(lds_optin_all(160 * 1024, &k_colfilter_lane4<0, true>, &k_colfilter_lane4<1, true>, &k_colfilter_lane4<1, false>,
                                 &k_colfilter_lane4<2, false>, &k_colfilter_lane4<2, true>));
            const auto kern = k.src == ColSrc::PackedFlags ? (divide ? &k_colfilter_lane4<2, true> : &k_colfilter_lane4<2, false>)
                                                           : (divide ? &k_colfilter_lane4<1, true> : &k_colfilter_lane4<1, false>);
            hipLaunchKernelGGL(kern, dim3((unsigned)cdiv(C, 16), (unsigned)j.W, 2), dim3(64), (size_t)lane4_ring_capacity(rad) * 64 * sizeof(float), r.st,
                               inW, inO, j.srcData, j.srcFlags, j.dstW, j.dstO, n, C, rad, denom, in_ws, j.sws, j.dws);
            break;
        }
        case ColFamily::LdsRing: {
            HIPCHK(lds_optin_all(160 * 1024, &k_colfilter_lds<0, true, false>, &k_colfilter_lds<1, true, false>, &k_colfilter_lds<1, false, false>,
                                 &k_colfilter_lds<1, true, true>, &k_colfilter_lds<2, false, false>, &k_colfilter_lds<2, true, false>));
            auto kern = &k_colfilter_lds<0, true, false>;
            if (k.src == ColSrc::PackedFlags) kern = divide ? &k_colfilter_lds<2, true, false> : &k_colfilter_lds<2, false, false>;
            else if (k.transposed) kern = &k_colfilter_lds<1, true, true>;
            else if (k.src == ColSrc::Images) kern = divide ? &k_colfilter_lds<1, true, false> : &k_colfilter_lds<1, false, false>;
            hipLaunchKernelGGL(kern, dim3((unsigned)cdiv(C, k.bt), (unsigned)j.W, 2), dim3(k.bt), (size_t)4 * 2 * rad * k.bt * sizeof(float), r.st,
                               inW, inO, j.srcData, j.srcFlags, j.dstW, j.dstO, n, C, rad, denom, in_ws, j.sws, j.dws, k.intw ? 1 : 0);
            break;
        }
        case ColFamily::MultiPass: {
            const int blk = C >= 256 ? 256 : (C >= 128 ? 128 : 64);
            const auto kern = k.src == ColSrc::ByteFlags ? &k_colfilter<0> : &k_colfilter<1>;
            hipLaunchKernelGGL(kern, dim3((unsigned)cdiv(C, blk), (unsigned)j.W, 2), dim3(blk), 0, r.st, j.bufW, j.bufO, j.srcData, j.srcFlags,
                               j.dstW, j.dstO, n, C, rad, denom, j.bws, j.sws, j.dws);
            break;
        }
        case ColFamily::MultiPassUnpadded:
            return set_err(TRI_EUNSUPPORTED, "radius %d takes the in-place multi-pass filter, which needs images padded to n + 4r rows", rad);
    }
    LAUNCHCHK();
    return TRI_OK;
}

// ---- frequency-axis stage: pick ---------------------------------------------------------------------------------------
enum class FreqStage {
    ExactRows,        // K4x: rows of the time stage's TF images in, rows out, then to FT
    FusedRing,        // K4r / K4qf + masked division in one kernel (launch_boxf)
    FusedLds,         // four LDS rings + masked division in one kernel (launch_colfilter_tf)
    LdsDiv,           // four LDS rings from the TF images, then the division (launch_colfilter_t)
    Lane4Div,         // lane per stage from the TF images, then the division (launch_colfilter_t)
    Transposed        // two transposes, launch_colfilter on the FT images (none at r = 0), then the division
};

// The frequency stage of one radius.  Shared by the flagger and tri_bench_boxfilter.
struct FreqPick {
    FreqStage route = FreqStage::Transposed;
    bool pipe = false;      // FusedRing: K4qf (the eight-wave stage pipeline) instead of K4r
    int ks = 0, B = 0;      // FusedRing: register slots of K4r / K4qf; K4qf: block length
    int xl = 0;             // ExactRows: code of the K4x instantiation (BoxxCodes)
    size_t off = 0;         // Transposed: first element of the FT images (rows [4r, 4r + n) of the padded buffers for the in-place
                            // multi-pass filter, rows [0, n) for the single-sweep one)
    ColPick col;            // Transposed, r > 0: the filter of the FT images
    bool defers = false;    // the stage leaves its division by float32(d)**4 to the masked division that follows it
};

// Frequency-axis stages that read the time-axis stage's TF images directly: four LDS rings at 128 threads (k_colfilter_lds_t),
// the same fused with the masked division (k_colfilter_lds_tf), lane per stage (k_colfilter_lane4<3, *>, radii 17..LANE4_R_MAX)
static bool colfilter_t_usable(const BoxRoutes& b, int rad) { return b.t_in && rad > 0 && rad <= 16; }
static bool colfilter_tf_usable(const BoxRoutes& b, int rad) { return b.fused_div && colfilter_t_usable(b, rad); }
static bool colfilter_t4_usable(const BoxRoutes& b, int rad) { return b.t_in && colfilter_use_lane4(b, rad); }

// lines of n positions, C of them in each of W windows
static FreqPick pick_freq_unfused(const BoxRoutes& b, int rad, int n, int C, int64_t W) {
    FreqPick p;
    p.off = colfilter_lds_block(b, rad, C) > 0 ? 0 : (size_t)4 * rad * C;
    if (rad > 0) p.col = pick_col_filter(b, ColSrc::Images, 0, true, rad, n, C, W, false);
    p.defers = rad > 0 && p.col.defers;
    return p;
}
// mode 1: |data - background| out; mode 2 (final pass): background, residual and NaN markers out.  srcW / srcO: the weight
// image and the data image of a window, lines n floats apart, windows sws_img floats apart.  exact_rows: K4x may be taken.
static FreqPick pick_freq_stage(const BoxRoutes& b, int mode, int rad, int n, int C, int64_t W, const float* srcW, const float* srcO,
                                size_t sws_img, bool exact_rows) {
    FreqPick p;
    const size_t gap = (size_t)(srcO - srcW);
    // register-ring fused stage: signed 32-bit buffer offsets, one descriptor over both images of a window
    const bool one_descriptor = ((uint64_t)gap + (uint64_t)n * C) * 4u < (1ull << 31);
    const int ks = one_descriptor ? boxr_pick_ks_f(b, rad) : 0;
    // exact row filter where the stage pipelines end
    p.xl = (rad > 0 && (!ks || rad >= BOXX_MIN_R) && exact_rows) ? boxx_pick_l(b, rad, n) : 0;
    if (p.xl > 0) { p.route = FreqStage::ExactRows; return p; }
    if (ks > 0) {
        p.route = FreqStage::FusedRing; p.ks = ks;
        // Few, long lines (an SKA slab: 64 windows of 512 lines x 65536 channels): the one-wave-per-32-lines kernels (K4r) fill
        // half the machine at best; the stage pipeline (a workgroup of eight waves per 64 lines) then takes the small radii too.
        const bool few = (int64_t)W * cdiv(C, 32) < BOXQF_FEW_WAVES;
        const bool want = b.pipe_f == Want::Forced || (b.pipe_f == Want::Auto && (2 * rad >= BOXQF_MIN_2R || (few && 2 * rad >= 16)));
        if (want && boxq_pick_ks(rad) > 0 && srcO > srcW && n % 4 == 0 && sws_img % 4 == 0 && gap % 4 == 0 && ((uintptr_t)srcW % 16 == 0) &&
            one_descriptor && (uint64_t)n * (uint64_t)C * 4u < (1ull << 31)) {
            p.pipe = true;
            // blocks of 8 positions (two workgroups per CU) while the delay line leaves the registers for it
            const bool b8 = b.pipe_f_b8 && 2 * rad >= 16 && 2 * rad < BOXQF_B8_MAX2R && boxqf_b8_exists(2 * rad / 8 * 8, mode);
            p.B = b8 ? 8 : 16;
            p.ks = b8 ? 2 * rad / 8 * 8 : boxq_pick_ks(rad);
        }
        return p;
    }
    if (colfilter_tf_usable(b, rad)) { p.route = FreqStage::FusedLds; return p; }
    if (colfilter_t_usable(b, rad)) { p.route = FreqStage::LdsDiv; p.defers = true; return p; }
    if (colfilter_t4_usable(b, rad)) { p.route = FreqStage::Lane4Div; p.defers = true; return p; }
    return pick_freq_unfused(b, rad, n, C, W);
}

// ---- frequency-axis stage: launch -----------------------------------------------------------------------------------
// Lines of n positions (ld floats apart in the source), C of them in each of W windows: the TF images (srcW, srcO) of the
// time stage in, FT images (dstW, dstO) out; `data` [C][n] and nanflag for the kernels that divide themselves.
struct FreqJob {
    const float *srcW = nullptr, *srcO = nullptr, *data = nullptr;
    float *dstW = nullptr, *dstO = nullptr;
    int n = 0, C = 0, ld = 0, rad = 0;
    size_t sws_img = 0, dws = 0, ws_data = 0;
    int64_t W = 1; uint8_t* nanflag = nullptr;
    // K4r, MODE 2: the residual a second time, as column panels [n / 64][C][64] where the kernel has the registers for it;
    // *wroteP is set when it wrote them (K4qf has no such output and leaves *wroteP alone)
    float* dstP = nullptr; size_t pws = 0; bool* wroteP = nullptr;
    // K4x: rows in, rows out -- (srcW, srcO) [C][ld] + data rows [C][n] (+ byte mask rows) -> outA (MODE 1: |data - bg|; MODE 2:
    // bg), outB (MODE 2: data - bg), rows [C][ld]; the outputs may alias the inputs (a workgroup has its whole line in LDS
    // before it writes); stats: optional pass counters
    const uint8_t* mask = nullptr; size_t ws_mask = 0;
    float *outA = nullptr, *outB = nullptr; size_t ws_outA = 0, ws_outB = 0; unsigned long long* stats = nullptr;
};

// k_colfilter_lds_t / k_colfilter_lane4<3, *>: filter only
static int launch_colfilter_t(const Run& r, const FreqPick& p, const FreqJob& j) {
    const float denom = box_denominator(j.rad);
    if (p.route == FreqStage::LdsDiv) {
        const size_t lds = ((size_t)4 * 2 * j.rad * CFT_BT + (size_t)CFT_PF * (CFT_BT + 1)) * sizeof(float);
        HIPCHK(lds_optin_all(160 * 1024, &k_colfilter_lds_t<false>, &k_colfilter_lds_t<true>));
        const auto k = p.defers ? &k_colfilter_lds_t<false> : &k_colfilter_lds_t<true>;
        hipLaunchKernelGGL(k, dim3((unsigned)cdiv(j.C, CFT_BT), (unsigned)j.W, 2), dim3(CFT_BT), lds, r.st, j.srcW, j.srcO, j.dstW, j.dstO,
                           j.n, j.C, j.ld, j.rad, denom, j.sws_img, j.dws);
    } else {
        const size_t lds = ((size_t)lane4_ring_capacity(j.rad) * 64 + 32 * 17) * sizeof(float);
        HIPCHK(lds_optin_all(160 * 1024, &k_colfilter_lane4<3, false>, &k_colfilter_lane4<3, true>));
        const auto k = p.defers ? &k_colfilter_lane4<3, false> : &k_colfilter_lane4<3, true>;
        hipLaunchKernelGGL(k, dim3((unsigned)cdiv(j.C, 16), (unsigned)j.W, 2), dim3(64), lds, r.st, j.srcW, j.srcO, (const float*)nullptr,
                           (const uint8_t*)nullptr, j.dstW, j.dstO, j.n, j.C, j.rad, denom, j.sws_img, (size_t)j.ld, j.dws);
    }
    LAUNCHCHK();
    return TRI_OK;
}

// The same stage fused with the masked division that follows it (k_colfilter_lds_tf):
// MODE 1 leaves |data - background| in dstO, MODE 2 the background in dstO, the signed
// residual in dstW and the per-line NaN markers.
template <int MODE>
static int launch_colfilter_tf(const Run& r, const FreqJob& j) {
    const size_t lds = (size_t)2 * ((size_t)4 * 2 * j.rad * CFF_BT + (size_t)CFT_PF * (CFF_BT + 1)) * sizeof(float);
    HIPCHK(lds_optin_all(160 * 1024, &k_colfilter_lds_tf<MODE>));
    hipLaunchKernelGGL(k_colfilter_lds_tf<MODE>, dim3((unsigned)cdiv(j.C, CFF_BT), (unsigned)j.W), dim3(2 * CFF_BT), lds, r.st, j.srcW, j.srcO,
                       j.dstW, j.dstO, j.data, j.n, j.C, j.ld, j.rad, box_denominator(j.rad), j.sws_img, j.dws, j.ws_data, j.nanflag);
    LAUNCHCHK();
    return TRI_OK;
}

// Register-ring form of the fused stage (K4r, k_boxf): any radius boxr_pick_ks() accepts.
template <int KS, int MODE>
static int launch_boxf_ks(const Run& r, const FreqJob& j) {
    const BoxDenom denom = box_reciprocal(box_denominator(j.rad));
    const int d = 2 * j.rad - KS;
    // (the panel output only where the kernel has the registers for it: see boxf_panel_ok())
    float* const dstP = (MODE == 2 && j.n % 64 == 0 && boxf_panel_ok(KS, d > 0)) ? j.dstP : nullptr;
    if (dstP && j.wroteP) *j.wroteP = true;
    const size_t lds = ((size_t)4 * d * 64 + (size_t)2 * boxr_pf_f(KS) * boxf_nsub(KS) * boxf_ts(boxr_pf_f(KS) * boxf_nsub(KS))) * sizeof(float);
    // one descriptor per window spans both images: the data image must follow the weight image closely
    if (j.srcO <= j.srcW || ((uint64_t)(j.srcO - j.srcW) + (uint64_t)j.C * j.ld) * 4u >= (1ull << 31))
        return set_err(TRI_EUNSUPPORTED, "fused frequency stage: the data image must follow the weight image within 2^31 bytes");
    const unsigned gap = (unsigned)(j.srcO - j.srcW);
    HIPCHK(lds_optin_all(160 * 1024, &k_boxf<KS, true, MODE>));
    // 32 register slots: two waves per SIMD only pay while the LDS part leaves room for them (measured: r = 30,
    // 28 LDS slots: 10.0 ms per 252 windows at two waves per SIMD, 7.0 ms with the one-wave register budget)
    auto k = d > 0 ? &k_boxf<KS, true, MODE> : &k_boxf<KS, false, MODE>;
    if constexpr (KS == 32) {
        if (d > 14) { k = &k_boxf<KS, true, MODE, 1>; HIPCHK(lds_optin_all(160 * 1024, k)); }
    }
    hipLaunchKernelGGL(k, dim3((unsigned)cdiv(j.C, 32), (unsigned)j.W), dim3(64), lds, r.st, j.srcW, gap, j.dstW, j.dstO, j.data, j.n, j.C, j.ld,
                       j.rad, denom, j.sws_img, j.dws, j.ws_data, j.nanflag, dstP, j.pws);
    LAUNCHCHK();
    return TRI_OK;
}
template <int KS, int MODE, int B>
static int launch_boxqf_ks(const Run& r, const FreqJob& j) {
    HIPCHK(lds_optin_all(160 * 1024, &k_boxqf<KS, MODE, B>));
    hipLaunchKernelGGL((k_boxqf<KS, MODE, B>), dim3((unsigned)cdiv(j.C, 64), (unsigned)j.W), dim3(512), boxqf_lds_bytes(B, boxqf_dbl(KS, B)), r.st,
                       j.srcW, (unsigned)(j.srcO - j.srcW), j.dstW, j.dstO, j.data, j.n, j.C, j.ld, j.rad, box_reciprocal(box_denominator(j.rad)),
                       j.sws_img, j.dws, j.ws_data, j.nanflag);
    LAUNCHCHK();
    return TRI_OK;
}
template <int MODE>
static int launch_boxf(const Run& r, const FreqPick& p, const FreqJob& j) {
    const char* const no_pipe = "no stage-pipeline kernel for %d slots";
    if (!p.pipe) return with_constant(p.ks, BoxfKs{}, "no register-ring kernel for %d slots", [&](auto KS) { return launch_boxf_ks<KS(), MODE>(r, j); });
    if (p.B == 16) return with_constant(p.ks, BoxqKs16{}, no_pipe, [&](auto KS) { return launch_boxqf_ks<KS(), MODE, 16>(r, j); });
    return with_constant(p.ks, BoxqfKs8{}, no_pipe, [&](auto KS) {
        if constexpr (boxqf_b8_exists(KS(), MODE)) return launch_boxqf_ks<KS(), MODE, 8>(r, j);
        else return set_err(TRI_EINVAL, no_pipe, (int)KS());
    });
}

// K4x
template <int MODE>
static int launch_boxx(const Run& r, const FreqPick& p, const FreqJob& j) {
    const float *const srcW = j.srcW, *const srcO = j.srcO;
    if (srcO <= srcW || j.ld % 4 != 0 || j.sws_img % 4 != 0 || (uint64_t)(srcO - srcW) % 4 != 0 || ((uintptr_t)srcW % 16 != 0) ||
        ((uintptr_t)j.data % 16 != 0) || j.ws_data % 4 != 0 || ((uintptr_t)j.outA % 16 != 0) || j.ws_outA % 4 != 0 ||
        (j.mask && (((uintptr_t)j.mask % 4 != 0) || j.ws_mask % 4 != 0)) || (uint64_t)(srcO - srcW) > 0xffffffffull ||
        (MODE == 2 && (((uintptr_t)j.outB % 16 != 0) || j.ws_outB % 4 != 0)) || j.C > 65535 * 1024)
        return set_err(TRI_EUNSUPPORTED, "exact row filter: unaligned images");
    const unsigned gap = (unsigned)(srcO - srcW);
    return with_constant(p.xl, BoxxCodes{}, "no exact row filter for code %d", [&](auto CODE) {
        constexpr int NTI = CODE() >> 8, L = CODE() & 255;
        // (the kernel also has a few static LDS bytes -- __syncthreads_or -- so 160 KB of dynamic LDS is refused: ask for 159)
        const auto k = boxx_recip_ok(j.rad) ? &k_boxx<NTI, L, MODE, true> : &k_boxx<NTI, L, MODE, false>;
        HIPCHK(lds_optin_all(159 * 1024, k));
        hipLaunchKernelGGL(k, dim3((unsigned)j.C, (unsigned)j.W), dim3(2 * NTI), boxx_lds_bytes(NTI, L, j.rad), r.st, srcW, gap, j.data, j.mask,
                           j.outA, j.outB, j.n, j.ld, j.rad, box_reciprocal(box_denominator(j.rad)), j.sws_img, j.ws_data, j.ws_mask, j.ws_outA,
                           j.ws_outB, j.nanflag, j.stats);
        LAUNCHCHK();
        return (int)TRI_OK;
    });
}
