// Device-side pieces that more than one KDE kernel unit uses (kde_kernels.hip with kde_sweep_f16.inc, kde_moment.hip,
// kde_prepass.hip, kde_cdf.hip): the 2^x family, the MFMA traits, the fragment helpers and the box tests of the pruned sweeps.  Everything here is
// __forceinline__; the library is built without relocatable device code, so nothing with storage lives here.
#pragma once
#include "kde_kernels.hpp"

namespace pbn {

// Device pointers of the sweeps are typed as GLOBAL-address-space pointers.  A pointer that reaches a kernel through a record in
// memory (the grouped launches' per-unit table) is otherwise a generic pointer: its loads become flat_load, whose completion order
// against LDS traffic is unknown, so every wait is a full `s_waitcnt vmcnt(0) lgkmcnt(0)` - the prefetch of the next tile is waited
// for before the current one is used.  (The kernel-argument pointers of the stand-alone launches are inferred global anyway.)
#define PBN_GLOBAL __attribute__((address_space(1)))

typedef double d4 __attribute__((ext_vector_type(4)));
typedef float f4 __attribute__((ext_vector_type(4)));

// 2^r on [-1/2, 1/2]: interpolants at Chebyshev nodes (exp2_poly), and minimax polynomials on [0, 1) for the v_fract form
// of the sweep's main loop (exp2_f64_fract).  The DP units are the binding resource of the fp64 sweep (DESIGN.md
// "roofline"); every polynomial degree costs one of its ~42 DP instructions per (tile, group, 4 values).  The
// log-likelihood sweeps use degree 6 on [0, 1) pinned to p(0) = 1, p(1) = 2 (Remez on the relative error among such
// polynomials, tools/exp2_coeffs.py 6 pinned): max relative error 2.22e-9 per term, i.e. <= 2.3e-9 ABSOLUTE on a logl
// whatever the number of terms (the error of a sum of positive terms is bounded by the per-term bound) - 400x inside the
// 1e-6 parity bar.  The pinning keeps 2^x continuous across the integers, where v_fract wraps: the largest term of a KDE
// sum sits at x = bias + 0 exactly, and the free minimax of even degree (1.86e-9) has errors of opposite sign at the two
// ends - a jump of 3.7e-9 on that term under perturbations of the last ulp.  -DPBN_EXP2_DEGREE=7 restores 4.0e-11
// (free minimax: same sign at both ends), =8 1.07e-12 (v_rndne form).
// The weight kernels (CKDE::cdf / sample, UCV) always use degree 8: the UCV objective is a difference of two pair sums
// and amplifies per-term errors.
#ifndef PBN_EXP2_DEGREE
#define PBN_EXP2_DEGREE 6
#endif

template <int DEG>
__device__ __forceinline__ double exp2_poly(double r);
template <>
__device__ __forceinline__ double exp2_poly<8>(double r) {
    double p = 0x1.63d136366db24p-20;
    p = __builtin_fma(p, r, 0x1.00dc4a532fb8ep-16);
    p = __builtin_fma(p, r, 0x1.4308ac85aa947p-13);
    p = __builtin_fma(p, r, 0x1.5d8745a728441p-10);
    p = __builtin_fma(p, r, 0x1.3b2ab7181b755p-7);
    p = __builtin_fma(p, r, 0x1.c6b08dd6fd234p-5);
    p = __builtin_fma(p, r, 0x1.ebfbdff823cedp-3);
    p = __builtin_fma(p, r, 0x1.62e42fef84cf0p-1);
    return __builtin_fma(p, r, 0x1.0000000000000p+0);
}
template <>
__device__ __forceinline__ double exp2_poly<7>(double r) {
    double p = 0x1.00c0e56000f6ep-16;
    p = __builtin_fma(p, r, 0x1.446c79f27429dp-13);
    p = __builtin_fma(p, r, 0x1.5d8775970d4b9p-10);
    p = __builtin_fma(p, r, 0x1.3b29d8bb04b01p-7);
    p = __builtin_fma(p, r, 0x1.c6b08da70e83cp-5);
    p = __builtin_fma(p, r, 0x1.ebfbe0aa03e9fp-3);
    p = __builtin_fma(p, r, 0x1.62e42fef9cc4fp-1);
    return __builtin_fma(p, r, 0x1.ffffffffa7138p-1);
}

// the leading coefficient of the degree-7 polynomial as a register operand: v_fma_f64 reads one scalar/literal only, so
// the first step C7 r + C6 needs one of the two in a VGPR; a caller that pins it once (pin_top) saves the v_mov the
// compiler otherwise re-materialises per 4 values
__device__ __forceinline__ double pin_top() {
    double c;
    asm volatile("v_mov_b64 %0, %1" : "=v"(c) : "s"(0x1.00c0e56000f6ep-16));
    return c;
}
__device__ __forceinline__ double exp2_f64_top(double x, double top) {
    double nf = __builtin_rint(x);
    double r = x - nf;
    double p = __builtin_fma(top, r, 0x1.446c79f27429dp-13);
    p = __builtin_fma(p, r, 0x1.5d8775970d4b9p-10);
    p = __builtin_fma(p, r, 0x1.3b29d8bb04b01p-7);
    p = __builtin_fma(p, r, 0x1.c6b08da70e83cp-5);
    p = __builtin_fma(p, r, 0x1.ebfbe0aa03e9fp-3);
    p = __builtin_fma(p, r, 0x1.62e42fef9cc4fp-1);
    p = __builtin_fma(p, r, 0x1.ffffffffa7138p-1);
    int n;
    asm("v_cvt_i32_f64 %0, %1" : "=v"(n) : "v"(nf));
    return __builtin_ldexp(p, n);
}

// 2^x for the sweep's main loop, 10 instructions instead of 11: the caller keeps its exponents biased by
// PBN_EXP2_BIAS (folded into the per-query constant, so free), which makes every value that matters non-negative; then
// v_fract_f64 is the whole range reduction (f = x - floor(x), exact) and the truncating v_cvt_i32_f64 of x itself is
// floor(x) - no v_rndne / subtract pair.  Degree-7 minimax (relative, Remez: tools/exp2_coeffs.py 7 0 1) on [0, 1):
// 4.02e-11.  A negative x (a term below 2^-128 of its query's sum, which holds a term >= 2^0) comes out at most 2x too
// large: invisible (N * 2^-128 relative); x <= -2^31 saturates to INT_MIN and gives 0 like the general form.
#define PBN_EXP2_BIAS 128.0
#if PBN_EXP2_DEGREE == 6
#define PBN_FRACT_TOP 0x1.c765a82c535bdp-13
#else
#define PBN_FRACT_TOP 0x1.68b07e4ac7b5bp-16
#endif
__device__ __forceinline__ double pin_top_fract() {
    double c;
    asm volatile("v_mov_b64 %0, %1" : "=v"(c) : "s"(PBN_FRACT_TOP));
    return c;
}
// FAST: 2^f of the FRACTION on the fp32 transcendental unit instead of the fp64 polynomial - fract, cvt_i32, cvt_f32_f64, v_exp_f32,
// cvt_f64_f32, ldexp: 6 instructions (v_exp_f32 holds the issue port for two slots) instead of 9.  f in [0, 1) converts to float with
// <= 6e-8 absolute error, v_exp_f32 is good to 1 ulp of a value in [1, 2]: <= 1.4e-7 relative per term (measured on C2: 5e-8 absolute
// on a logl at worst, 1e-10 relative on the slogl) instead of 2.2e-9 - and a sum of positive terms moves by at most the per-term
// bound.  Like the pinned polynomial it is continuous across the integers (f = 0 gives exactly 1; an f that rounds to 1.0f gives
// exactly 2) and, with integer offsets, a function of the (row, query) pair only: sums taken in different partitions still agree to
// rounding.  Used by the sweeps whose result is a SUM over the test rows (slogl, the score engine's terms: the north star's bar is
// 1e-6 relative on slogl); per-row logl outputs keep the polynomial (SweepArgs::fast).  C2 51.5 -> 46.3 ms, cv64 3.42 -> 3.06 s,
// bounded C3 15.7 -> 14.0 s (profiles/r4/expf32_probe.txt).  -DPBN_EXP2_F32=0 compiles it out.
// Round 6: the plain sum-only sweeps (every shape but the fused CKDE ones) take exp2_magic below instead - the same v_exp_f32, fed from the
// accumulator's own words; this form stays for the fused conditional sweeps and for -DPBN_EXP2_MAGIC=0.
#ifndef PBN_EXP2_F32
#define PBN_EXP2_F32 1
#endif
template <bool FAST = false>
__device__ __forceinline__ double exp2_f64_fract(double x, double top) {
    const double f = __builtin_amdgcn_fract(x);      // v_fract_f64
    int n;
    asm("v_cvt_i32_f64 %0, %1" : "=v"(n) : "v"(x));  // truncation = floor for x >= 0; saturating
    if constexpr (FAST && PBN_EXP2_F32) {
        (void)top;
        return __builtin_ldexp((double)__builtin_amdgcn_exp2f((float)f), n);
    }
#if PBN_EXP2_DEGREE == 6
    double p = __builtin_fma(top, f, 0x1.46214fe0d40c9p-10);
    p = __builtin_fma(p, f, 0x1.3d217bf137896p-7);
    p = __builtin_fma(p, f, 0x1.c686b389d4c31p-5);
    p = __builtin_fma(p, f, 0x1.ebfd7378d3f76p-3);
    p = __builtin_fma(p, f, 0x1.62e42af6f5a89p-1);
    p = __builtin_fma(p, f, 1.0);
#else
    double p = __builtin_fma(top, f, 0x1.2cfd657b74f58p-13);
    p = __builtin_fma(p, f, 0x1.5fddc72ac74dep-10);
    p = __builtin_fma(p, f, 0x1.3b0838502e0f5p-7);
    p = __builtin_fma(p, f, 0x1.c6b2b0142cedbp-5);
    p = __builtin_fma(p, f, 0x1.ebfbcf8c8da34p-3);
    p = __builtin_fma(p, f, 0x1.62e4301f16f2dp-1);
    p = __builtin_fma(p, f, 0x1.ffffffffa7934p-1);
#endif
    return __builtin_ldexp(p, n);
}

// MAGIC (round 6): the 2^x of sum-only fp64 sweeps without a single DP instruction of range reduction.  The per-query constant that
// starts the MFMA accumulator carries PBN_MAGIC_C = 1.5 * 2^20 - 1 + 2^-24 on top of the biased exponent, so the MFMA chain itself leaves
// y = 1.5 * 2^20 + (x - 1 + 2^-24): a double of FIXED exponent whose mantissa is x in fixed point - the low word is the fraction (32
// bits), the high word is 0x41380000 + floor(x - 1 + 2^-24).  Then
//   u  = v_alignbit_b32(0x7f, y.lo, 9)      the float 1 + f, f = the fraction's top 23 bits (the 2^-24 in the constant makes the cut
//                                            a round-to-nearest of x: +-2^-24, no bias);
//   e  = v_exp_f32(u) in [2, 4]              = 2^(1 + f), 1 ulp;
//   ed = v_cvt_f64_f32(e);  ed.hi += n << 20 (v_lshl_add_u32; n = y.hi clamped by v_med3_i32 to 0x41380000 - 1024 ... + 1023)
// = 2^x in 6 instructions / 7 issue slots with the sum's FMA, against 7 / 8 of the v_fract form (fract, cvt_i32, cvt_f32, exp, cvt_f64,
// ldexp, fma).  The clamp makes the form total: the exponent field of ed (1024 or 1025) + n stays inside [0, 2047] - n = -1024 gives a
// subnormal or 2^-1022 (a term 2^-1150 below its sum), n = 1023 gives NaN or inf, which the sums' overflow tests catch exactly like the
// inf of the v_fract form; an accumulator outside [2^20, 2^21) - |x| beyond 2^19, NaN, inf - has a high word beyond the clamp's ends and
// comes out as ~0 (x -> -inf) or NaN (everything else).  Accuracy per term: x on a 2^-32 grid (the MFMA chain rounds there: <= 1e-9),
// f to 2^-24 (4.1e-8 relative), v_exp_f32 1 ulp of a value in [2, 4] (<= 1.2e-7): <= 1.65e-7, against 1.4e-7 of the v_fract form.
// Like that form it is a function of the (row, query) pair alone: the offsets are integers, and an integer added to y moves the high
// word only (the grid and every rounding of the chain stay where they are while y stays in its binade).
#ifndef PBN_EXP2_MAGIC
#define PBN_EXP2_MAGIC 1
#endif
#ifndef PBN_MAGIC_CLAMP
#define PBN_MAGIC_CLAMP 1   // 0: probe builds only (the unclamped 5-instruction form: wraps on exponents beyond +-1023)
#endif
#ifndef PBN_MAGIC_PRUNED
#define PBN_MAGIC_PRUNED 1   // the pruned / grouped sum-only sweeps too (their far tiles pay one v_add_f64 per value to take the constant off)
#endif
#ifndef PBN_MAGIC_GUARD
#define PBN_MAGIC_GUARD 1   // unpruned sweeps: chunks whose exponents are proven inside +-1022 skip the clamp (kde_sweep_body: GUARD)
#endif
#define PBN_MAGIC_C (0x1.8p20 - 1.0 + 0x1p-24)
#define PBN_MAGIC_H0 0x41380000
template <bool CLAMP = true>
__device__ __forceinline__ double exp2_magic(double y) {
    const unsigned lo = (unsigned)__double2loint(y);
    int t = __double2hiint(y);
    const float u = __uint_as_float(__builtin_amdgcn_alignbit(0x7fu, lo, 9));
    const double ed = (double)__builtin_amdgcn_exp2f(u);
    if constexpr (CLAMP) {
        t = t < PBN_MAGIC_H0 - 1024 ? PBN_MAGIC_H0 - 1024 : t;
        t = t > PBN_MAGIC_H0 + 1023 ? PBN_MAGIC_H0 + 1023 : t;   // (v_med3_i32)
    }
    unsigned h2;
    if constexpr (CLAMP) h2 = (unsigned)__double2hiint(ed) + ((unsigned)t << 20);
    else asm("v_lshl_add_u32 %0, %1, 20, %2" : "=v"(h2) : "v"(t), "v"(__double2hiint(ed)));   // (left to the compiler this becomes three 64-bit operations)
    return __hiloint2double((int)h2, __double2loint(ed));
}

template <int DEG>
__device__ __forceinline__ double exp2_f64(double x) {
    // x <= ~1000 (larger values are caught by the overflow check of the caller), any negative value.
    double nf = __builtin_rint(x);  // v_rndne_f64
    double r = x - nf;              // exact
    const double p = exp2_poly<DEG>(r);
    int n;
    asm("v_cvt_i32_f64 %0, %1" : "=v"(n) : "v"(nf));  // saturating: -1e30 -> INT_MIN -> ldexp gives 0
    return __builtin_ldexp(p, n);                      // v_ldexp_f64
}

template <typename T>
struct Tr;
template <>
struct Tr<double> {
    using vec4 = d4;
    static __device__ __forceinline__ vec4 mfma(double a, double b, vec4 c) {
        return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0);
    }
    static constexpr int GEN_DEG = PBN_EXP2_DEGREE < 7 ? 7 : PBN_EXP2_DEGREE;   // rare paths: v_rndne form, degree >= 7
    static __device__ __forceinline__ double ex2(double x) { return exp2_f64<GEN_DEG>(x); }
    static __device__ __forceinline__ double top() { return PBN_EXP2_DEGREE <= 7 ? pin_top_fract() : 0.0; }
    // main-loop form: x carries bias() (see exp2_f64_fract)
    template <bool FAST = false>
    static __device__ __forceinline__ double ex2p(double x, double top) {
        return PBN_EXP2_DEGREE <= 7 ? exp2_f64_fract<FAST>(x, top) : exp2_f64<GEN_DEG>(x);
    }
    static __device__ __forceinline__ double bias() { return PBN_EXP2_BIAS; }
    // MAGIC sweeps (exp2_magic): the constant on top of the biased exponents, and 2^x from such an accumulator
    static __device__ __forceinline__ double magic() { return PBN_MAGIC_C; }
    template <bool CLAMP = true>
    static __device__ __forceinline__ double ex2m(double y) { return exp2_magic<CLAMP>(y); }
    static __device__ __forceinline__ double ex2_hi(double x) { return exp2_f64<8>(x); }
    static __device__ __forceinline__ double big() { return 0x1p900; }
    // C/D row held by (lane group lg, register i): cdna_hip_programming.md §3 "f64 MFMA"
    static __host__ __device__ __forceinline__ int crow(int lg, int i) { return lg + 4 * i; }
};
template <>
struct Tr<float> {
    using vec4 = f4;
    static __device__ __forceinline__ vec4 mfma(float a, float b, vec4 c) {
        return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
    }
    static __device__ __forceinline__ float ex2(float x) { return __builtin_amdgcn_exp2f(x); }  // v_exp_f32
    static __device__ __forceinline__ float ex2_hi(float x) { return __builtin_amdgcn_exp2f(x); }
    static __device__ __forceinline__ float top() { return 0.0f; }
    template <bool FAST = false>
    static __device__ __forceinline__ float ex2p(float x, float) { return __builtin_amdgcn_exp2f(x); }
    static __device__ __forceinline__ float bias() { return 0.0f; }
    static __device__ __forceinline__ float magic() { return 0.0f; }
    template <bool CLAMP = true>
    static __device__ __forceinline__ float ex2m(float y) { return __builtin_amdgcn_exp2f(y); }
    static __device__ __forceinline__ float big() { return 0x1p100f; }
    static __host__ __device__ __forceinline__ int crow(int lg, int i) { return 4 * lg + i; }
};

#define PBN_PAD_NORM (-1e30)

template <typename T>
__device__ __forceinline__ T max4(typename Tr<T>::vec4 v) {
    T a = v[0] > v[1] ? v[0] : v[1];
    T b = v[2] > v[3] ? v[2] : v[3];
    return a > b ? a : b;
}
template <typename T>
__device__ __forceinline__ T colmax(T v) {  // max over the 4 lanes (lane>>4 = 0..3) that share a query column
    T o = __shfl_xor(v, 16);
    v = v > o ? v : o;
    o = __shfl_xor(v, 32);
    return v > o ? v : o;
}

// XCD-aware block order (cdna_hip_programming.md T1, bijective form): workgroups are handed round-robin to the 8 XCDs, so
// `linear id % 8` labels the blocks that share an L2.  The remap gives every XCD a CONTIGUOUS range of the logical
// (split-major) grid: all blocks resident on an XCD sweep the same training split, which then lives in that XCD's 4 MB
// L2 instead of being re-fetched through the fabric by every query block.  Pure placement - results do not depend on it.
__device__ __forceinline__ void xcd_block(int& qx, int& split) {
    const unsigned gx = gridDim.x, nwg = gx * gridDim.y;
    const unsigned bid = blockIdx.x + gx * blockIdx.y;
    const unsigned xcd = bid & 7u, q = nwg >> 3, r = nwg & 7u;
    const unsigned wg = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (bid >> 3);
    qx = (int)(wg % gx);
    split = (int)(wg / gx);
}

// Tile pruning, lane-parallel: lane l tests training tile tb + l against the box of the wave's queries (squared distance
// between the boxes puts every exponent of the tile below the wave's bound -> skip), one ballot gives the visit mask of 64
// tiles.  The sweeps then walk the set bits only: a skipped tile costs 1/64 of a test and no fragment load (the first
// version tested tile by tile on wave-uniform values - 15 DP instructions and three loads per tile, skipped or not:
// a fifth of a kept tile's cost in the fp32 sweep and ALL of a skipped tile's).
template <int PD, typename BP>
__device__ __forceinline__ unsigned long long prune_visit_mask(BP tile_box, int pd, int64_t tb, int64_t t1,
                                                               const double (&wlo)[PD], const double (&whi)[PD], double wthr, int lane) {
    const int64_t t = tb + lane;
    bool keep = false;
    if (t < t1) {
        const BP bx = tile_box + t * 2 * pd;
        double d2 = 0.0;
#pragma unroll
        for (int k = 0; k < PD; ++k)
            if (k < pd) {
                const double g1 = bx[k] - whi[k], g2 = wlo[k] - bx[pd + k];
                double g = g1 > g2 ? g1 : g2;
                g = g > 0.0 ? g : 0.0;
                d2 = __builtin_fma(g, g, d2);
            }
        keep = !(-0.5 * d2 < wthr);
    }
    return __ballot(keep);
}

// The same test against ONE 16-query group's own box and bound (fp64 pruned sweeps): a wave owns QG groups, consecutive in Morton
// order, and the box of all of them is up to twice as wide per axis as a group's own - at 3-4 dimensions, where a wave's box is
// as wide as the kernel's support, a third of the (tile, group) pairs of a visited tile lie beyond the group's own support.  The
// boxes are re-read per group so that no box stays in registers across the walk: the tile's box from L1 / L2 and the group's own box - a uniform
// address, but a VECTOR load per lane all the same (the kernel holds atomics and stores, so the compiler does not prove the memory unclobbered and
// emits no scalar load) - or, in the d = 8 shape, from the copy the wave keeps in LDS (kde_sweep_body: QLDS).  `pd` is a compile-time constant
// in that shape (PDFIX): the loop below is then flat, every load of the test issued before the first wait.
template <int PD, typename BP, typename QP>
__device__ __forceinline__ unsigned long long prune_group_mask(BP tile_box, QP qbox, int pd, int64_t tb, int64_t t1, double thr, int lane) {
    const int64_t t = tb + lane;
    bool keep = false;
    if (t < t1) {
        const BP bx = tile_box + t * 2 * pd;
        double d2 = 0.0;
#pragma unroll
        for (int k = 0; k < PD; ++k)
            if (k < pd) {
                const double g1 = bx[k] - qbox[pd + k], g2 = qbox[k] - bx[pd + k];
                double g = g1 > g2 ? g1 : g2;
                g = g > 0.0 ? g : 0.0;
                d2 = __builtin_fma(g, g, d2);
            }
        keep = !(-0.5 * d2 < thr);
    }
    return __ballot(keep);
}

// One uniform test per (64-tile batch, query group): does the batch's box come within the drop threshold of the group's box at all?
template <int PD, typename BP, typename QP>
__device__ __forceinline__ bool batch_in_reach(BP bb, QP qbox, int pd, double thr) {
    double d2 = 0.0;
#pragma unroll
    for (int k = 0; k < PD; ++k)
        if (k < pd) {
            const double g1 = bb[k] - qbox[pd + k], g2 = qbox[k] - bb[pd + k];
            double g = g1 > g2 ? g1 : g2;
            g = g > 0.0 ? g : 0.0;
            d2 = __builtin_fma(g, g, d2);
        }
    return !(-0.5 * d2 < thr);
}

// ... and with the MOMENT pass (round 5): `mom` = the (tile, group) pairs whose contribution is taken from the tile's moments instead
// (kde_moment_group_kernel).  The tile's rows are z_t = c + delta_t, |delta_t| <= rho; for a query at u = z_q - c a row's term is
// 2^(-|u|^2 / 2) 2^(-|delta_t|^2 / 2) e^(s_t), s_t = a u.delta_t, a = ln 2, and e^s is replaced by its Taylor polynomial T_P(s).  By Lagrange's
// remainder |e^s - T_P(s)| <= |s|^(P+1) / (P+1)! max(1, e^s), so the row's error is at most |s|^(P+1) / (P+1)! times the larger of its own term
// and 2^(-|u|^2 / 2 - |delta_t|^2 / 2) - and BOTH are at most 2^(-d2min / 2), d2min the smallest distance between the tile's and the group's box (the
// centroid lies in the tile's box).  With |s| <= w = a |u|max rho (|u|max: the largest distance between the two boxes) a tile whose terms lie 2^E below the
// group's sum bound may therefore be expanded when E + log2(w^(P+1) / (P+1)!) <= -(margin + PBN_MOM_EXTRA): all expanded tiles together then err by at
// most N 2^-(margin + extra) of a sum - a quarter of what pruning may drop.  The bound is proved, the realised error is 5-6 orders smaller
// (tools/moment_prototype.py: 2e-13 of a sum on C3's folds).  Near tiles qualify through small |u|, far ones through small terms; the middle
// distances are what stays with the sweep.  Both kernels classify with this one function on the same inputs, so every (tile, group) pair is
// taken by exactly one of them.
#ifndef PBN_MOM_EXTRA
#define PBN_MOM_EXTRA 2.0
#endif
template <int PD, typename BP, typename RP>
__device__ __forceinline__ unsigned long long prune_group_mask3(BP tile_box, BP qbox, RP rad2, int pd, int64_t tb, int64_t t1, double thr, double thr_near,
                                                                double thr_mom, int lane, unsigned long long& near, unsigned long long& mom) {
#pragma clang fp contract(off)   // both kernels must take bit-identical decisions: no fused multiply-adds the inliner could place differently
    const int64_t t = tb + lane;
    bool keep = false, kn = false, km = false;
    if (t < t1) {
        const BP bx = tile_box + t * 2 * pd;
        double d2 = 0.0, f2 = 0.0;
#pragma unroll
        for (int k = 0; k < PD; ++k)
            if (k < pd) {
                const double g1 = bx[k] - qbox[pd + k], g2 = qbox[k] - bx[pd + k];
                double g = g1 > g2 ? g1 : g2;
                g = g > 0.0 ? g : 0.0;
                d2 = __builtin_fma(g, g, d2);   // (explicit fmas are kept as written)
                const double h1 = bx[pd + k] - qbox[k], h2 = qbox[pd + k] - bx[k];
                const double h = h1 > h2 ? h1 : h2;
                f2 = __builtin_fma(h, h, f2);
            }
        const double ex = -0.5 * d2;
        keep = !(ex < thr);
        kn = !(ex < thr_near);
        // w = ln 2 * |u|max * rho, rounded up; log2(w^9 / 9!) = 9 log2 w - log2 9! (v_sqrt_f32 / v_log_f32: 1 ulp, covered by the + 0.02)
        const float w = 0.69314724f * __builtin_amdgcn_sqrtf((float)f2 * 1.000001f * rad2[t]) * 1.000001f;
        const float logr = (float)(PBN_MOM_ORDER + 1) * __builtin_amdgcn_logf(w) - PBN_MOM_LOG2_FACT + 0.02f;
        km = keep && ((double)logr + ex <= thr_mom);
    }
    near = __ballot(kn);
    mom = __ballot(km);
    return __ballot(keep);
}

// The grid of a pruned sweep is one-dimensional and split-major (the workgroups in flight share a split's fragments in L2),
// with the splits taken from both ends of the Morton order inwards: the corner splits - sparse regions, where a query's
// whole neighbourhood lies in its own split and the workgroup visits nearly all of its tiles - start first.  Pure placement.
// (Measured and dropped: every query group's nearest splits first - all splits in flight at once, the L2 sharing is gone.)
__device__ __forceinline__ void pruned_block(const SweepArgs& a, int groups_per_block, unsigned b, int& qx, int& split) {
    const unsigned Gq = (unsigned)((a.nqtiles + groups_per_block - 1) / groups_per_block), Gs = (unsigned)a.nsplit_grid;
    const unsigned k = b / Gq;
    qx = (int)(b % Gq);
    split = (k & 1u) ? (int)(Gs - 1 - (k >> 1)) : (int)(k >> 1);
}

}  // namespace pbn
