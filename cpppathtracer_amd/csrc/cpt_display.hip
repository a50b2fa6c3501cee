// cpt_display.hip — the display path of the MI355X integrator (gfx950, wave64).
//
//   dn_weight_slow*, dn_exp_short, dn_near_midpoint, dn_weights, dn_pair_*, g_dn_exp_table
//                         the display weight min(exp(-d2/M_PI), 1.0) (path_tracer.cu:215-233)
//   k_selftest_dn_weight  its exhaustive check (cpt_selftest_qdiv which = 6, 7), beside the code
//                         it checks so the 8 KB table exists once
//   k_denoise_rows        Denoising + Mix (path_tracer.cu:177-254);  launch_denoise_mix
//                         <HOST, HIST>: HIST the same with a per-pixel Mix weight (cpt_denoise_mix_history)
//   k_fill_count          the count plane's fill;  launch_fill_count
//   k_stitch_rows         the row-tile gather (cpt_gather_rows);  launch_stitch_rows
//   k_stitch_moments      the gather of a source's adaptive moments;  launch_stitch_moments
//
// Reference semantics per function are cited inline; DESIGN.md has the data layout and the
// roofline of each kernel.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cpt_path.hpp"
#include "cpt_dn_exp.hpp"

namespace cpt {

// ======================================================================================
// Display path: Denoising + Mix (path_tracer.cu:177-254) fused into one stencil kernel.
//
// Input: the pass radiance (accumulator rgb / pass count) and first-hit normals of the
// last render; depth is the constant 1e30 (a18), so its weight is exp(0) = 1.  The
// reference's launch covers W' x H' = 16*floor(W/16) x 16*floor(H/16) pixels and indexes
// neighbours by LINEAR offset v*W' + u, so x +- 1, 2 wraps into the adjacent row and only
// offsets outside [0, W'*H') get zero weight (path_tracer.cu:205-216); reproduced here.
// Weights min(exp(-d2/M_PI), 1.0) are double (path_tracer.cu:215-222).  Mix:
// mix = lerp(mix, clamp(denoised, 0, 1), 1/cur_sample_idx); bytes 0..2 = 255.99*(b, g, r)
// (path_tracer.cu:241-254); the alpha byte, which the reference never writes (its frame copies
// whatever the device buffer held, :251-253,303), is stored as 0 in one 32-bit store.
// ======================================================================================
// min(exp(-(dist2) / M_PI), 1.0) in double, stored to float (path_tracer.cu:224,228,231), for a
// float dist2 -- the oracle's dm_exp(-(double)dist2 / REF_PI), branch-free.  The SLOW form (round 4),
// now only the fallback of dn_weights below near a float rounding boundary:
//  * dist2 in (0, 330): x = -dist2/pi in (-105.05, 0), the quotient from dm::div_pi's sequence
//    (correctly rounded: it depends only on dist2's significand, and every significand is
//    checked); then dm::exp's own steps -- k, the two-part reduction, the Horner polynomial --
//    and its ldexp, which for k in [-152, 0] is one exact multiplication by 2^k (v_ldexp_f64);
//  * dist2 == 0: exp(-0) = 1;  dist2 >= 330 (inf included): exp(x) < 2^-150, which rounds to
//    float 0;  NaN: exp(NaN) = NaN, and `w < 1.0 ? w : 1.0` gives 1.
// tests/test_exact_identities.py checks the whole function against the oracle's expression
// for every float in [0, 2341] and the special values.
__device__ __forceinline__ float dn_weight_slow_inl(float dist2) {
    constexpr double INV_PI = 1.0 / REF_PI;
    const double a = (double)dist2;
    const double q = a * INV_PI;
    const double x = -__builtin_fma(__builtin_fma(-q, REF_PI, a), INV_PI, q);
    const double k = __builtin_floor(__builtin_fma(x, dm::kc(dm::INV_LN2), 0.5));
    const double r = __builtin_fma(-k, dm::kc(dm::LN2_LO), __builtin_fma(-k, dm::kc(dm::LN2_HI), x));
    double p = 1.0 / 6227020800.0;
    p = __builtin_fma(r, p, dm::kc(1.0 / 479001600.0));
    p = __builtin_fma(r, p, dm::kc(1.0 / 39916800.0));
    p = __builtin_fma(r, p, dm::kc(1.0 / 3628800.0));
    p = __builtin_fma(r, p, dm::kc(1.0 / 362880.0));
    p = __builtin_fma(r, p, dm::kc(1.0 / 40320.0));
    p = __builtin_fma(r, p, dm::kc(1.0 / 5040.0));
    p = __builtin_fma(r, p, dm::kc(1.0 / 720.0));
    p = __builtin_fma(r, p, dm::kc(1.0 / 120.0));
    p = __builtin_fma(r, p, dm::kc(1.0 / 24.0));
    p = __builtin_fma(r, p, dm::kc(1.0 / 6.0));
    p = __builtin_fma(r, p, dm::kc(0.5));
    p = __builtin_fma(r, p, dm::kc(1.0));
    p = __builtin_fma(r, p, dm::kc(1.0));
    const double w = __builtin_ldexp(p, (int)k);
    float f = (float)(w < 1.0 ? w : 1.0);
    f = dist2 >= 330.0f ? 0.0f : f;
    return dist2 == 0.0f ? 1.0f : f;
}
// (out of line where a weight is evaluated alone; inlined in the batched weights, whose kernels
// would otherwise spill the caller-saved VGPRs live across the call)
__device__ __noinline__ float dn_weight_slow(float dist2) { return dn_weight_slow_inl(dist2); }


// The weight's short form (round 5): the same float, from a double approximation E' of
// exp(-dist2/pi) that is within 2^-46.3 (relative) of the oracle's double E, rounded to float
// only where that cannot matter:
//  * E' = 2^-(n>>S) * T[n & (N-1)] * P(r) (cpt_dn_exp.hpp: N = 2^S table entries, P of degree
//    DN_POLY_DEG):  z = dist2 * N/(pi ln2) (KN_HI + KN_LO), n = round(z) by the 1.5*2^52
//    shifter (n is t's low word), r = z - n in [-1/2, 1/2] (one fma against the exact product
//    dist2 * KN_HI, then the low part), T[j] = 2^(-j/N) correctly rounded from the LDS table,
//    P = the Taylor polynomial of 2^(-r/N), and 2^-(n>>S) applied to T's exponent field
//    (T >= 1/2 and n>>S <= 151: stays normal).  N = 1024, degree 3 (8 KB; truncation
//    < 2^-50.7); round 5's first table was N = 32, degree 5 (256 B, conflict-free in LDS,
//    truncation < 2^-48.7).  E' is within ~2^-48.5 of exp(-dist2/pi); the oracle's
//    E = dm_exp(RN(-dist2/pi)) is within 2^-47 (the quotient's rounding, |x| < 105.05) + 2^-52
//    of it.
//  * Guard (dn_near_midpoint): if no float rounding boundary lies within 2^-44 E' of E' (its
//    bits below float precision are not within 2^9 of the half-way pattern), every double in
//    between rounds alike, E included (rounding is monotone), so (float)E' is the oracle's float.
//    Otherwise (about 1 in 10^6 weights; also subnormal float results and NaN) the slow form
//    decides.  dist2 = 0 and dist2 >= 330 keep their shortcuts.
// tests/test_exact_identities.py restates it on the host against the oracle for every float in
// [0, 2341]; test_gpu_parity.py::test_dn_weight_exhaustive runs this device code against
// dn_weight_slow for all 2^31 non-negative float patterns.
__device__ const double g_dn_exp_table[DN_EXP_N] = CPT_DN_EXP_TABLE_INIT;

__device__ __forceinline__ double dn_exp_short(float dist2, const double* __restrict__ tab) {
    constexpr double SHIFT = 0x1.8p52;
    const double a = (double)dist2;
    const double t = __builtin_fma(a, DN_KN_HI, SHIFT);
    const double nd = t - SHIFT;
    const uint32_t n = (uint32_t)__double2loint(t);
    double r = __builtin_fma(a, DN_KN_HI, -nd);
    r = __builtin_fma(a, DN_KN_LO, r);
    double p = DN_POLY_DEG >= 4 ? (DN_POLY_DEG >= 5 ? __builtin_fma(r, DN_C5, DN_C4) : DN_C4) : DN_C3;
    if (DN_POLY_DEG >= 4) p = __builtin_fma(r, p, DN_C3);
    p = __builtin_fma(r, p, DN_C2);
    p = __builtin_fma(r, p, DN_C1);
    p = __builtin_fma(r, p, 1.0);
    const double T = tab[n & (uint32_t)(DN_EXP_N - 1)];
    const double Ts = __hiloint2double(__double2hiint(T) - (int)((n >> DN_EXP_SHIFT) << 20), __double2loint(T));
    return Ts * p;
}

// The guard on the bits of e: for e in [2^-126, 1] (a normal float result) rounding to float looks
// at the 29 mantissa bits below float precision, all in e's low word; e rounds like every double
// within 2^-44 e of it unless those bits lie within 2^9 (> 2^-44 / 2^-52 = 2^8 double ulps, with
// margin) of the half-way pattern 2^28.  Smaller e (a subnormal float result, dist2 > 274.5),
// larger e, NaN and inf are sent to the slow form, whose dist2 >= 330 shortcut the caller applies.
__device__ __forceinline__ bool dn_near_midpoint(double e) {
    const uint32_t lo = (uint32_t)__double2loint(e), hi = (uint32_t)__double2hiint(e);
    const int d = (int)(lo & 0x1fffffffu) - (1 << 28);
    const bool normal_f = hi >= 0x38100000u && hi <= 0x3ff00000u;   // 2^-126 <= e <= 1 (e > 0 here)
    return !normal_f || (d < 512 && d > -512);
}

// ---------------------------------------------------------------------------------------------
// k_denoise_rows (round 5, the default): the same Denoising + Mix, bit for bit, as a sliding
// window down a strip of columns (path_tracer.cu:177-254).
//  * A block owns a strip of 60 output columns (lanes 2..61 of each wave; lanes 0, 1, 62, 63 carry
//    the two halo columns each side) and a run of output rows.  Lane j of row Y holds the pixel of
//    LINEAR index L = Y W' + c0 - 2 + j: the stencil's v W' + u offsets (path_tracer.cu:205-216),
//    so columns past either edge wrap into the adjacent row exactly as the reference's do.
//  * When row R enters, the 12 pair weights whose later pixel is (R, j) are computed: the two
//    same-row pairs (R, j+1), (R, j+2) and the pairs with rows R-1 and R-2 at columns j-2..j+2 --
//    every unordered pair of the stencil exactly once -- into a ring of weights in LDS.
//  * Row O = R - 2 is then complete: each output lane sums its 25 taps in the reference's order,
//    reading the weights it needs from the ring (its own, or a neighbour's at lane j +- u).
// The weights are evaluated in batches of DN_BATCH with one wave-wide fallback branch
// (dn_weight's guard), so the batch's exp chains overlap.
constexpr int DNS_LANES = 64, DNS_COLS = 60;
struct DnsPix { float4 rgbv; float4 nd; };   // (r, g, b, valid), (nx, ny, nz, depth)
// The ring is two SoA arrays of float4 (16-B lane stride): a wave's ds_read_b128 at consecutive
// lanes then covers all 64 banks once per 16-lane group (MI355X_MICROARCH.md §LDS), where the
// 32-B pixel struct put two lanes of a group on the same banks (57% of LDS cycles were conflicts).

// Pair weights c_w * n_w * p_w of N pairs (path_tracer.cu:219-233; dn_pair_weight's factors, in
// the same order), batched: N short exps in flight, and the guard's rare fallback as one branch.
template <int N>
__device__ __forceinline__ void dn_weights(const float d2[N], float w[N], const double* __restrict__ tab) {
    uint32_t slow = 0;
#pragma unroll
    for (int i = 0; i < N; ++i) {
        const double e = dn_exp_short(d2[i], tab);
        w[i] = (float)e;
        slow |= dn_near_midpoint(e) && !(d2[i] >= 330.0f) ? 1u << i : 0u;
    }
    // the fallback, one call site per batch: each trip serves every lane's lowest pending weight
    while (__builtin_expect(__builtin_amdgcn_ballot_w64(slow != 0) != 0, 0)) {
        const int k = slow ? __builtin_ctz(slow) : -1;
        float x = 0.0f;
#pragma unroll
        for (int i = 0; i < N; ++i) x = k == i ? d2[i] : x;
        float r = 0.0f;
        if (k >= 0) r = dn_weight_slow_inl(x);
#pragma unroll
        for (int i = 0; i < N; ++i) w[i] = k == i ? r : w[i];
        slow &= slow - 1u;
    }
#pragma unroll
    for (int i = 0; i < N; ++i) {
        w[i] = d2[i] >= 330.0f ? 0.0f : w[i];
        w[i] = d2[i] == 0.0f ? 1.0f : w[i];
    }
}

// The three squared differences of one pair (path_tracer.cu:221-231): colour, normal (clamped at
// 0: (float)max((double)dn, 0.0), the reference's clamp in double), depth.
__device__ __forceinline__ void dn_pair_dist(const DnsPix& a, const DnsPix& b, float& c2, float& n2, float& p2) {
    v3 t = mk(a.rgbv.x, a.rgbv.y, a.rgbv.z) - mk(b.rgbv.x, b.rgbv.y, b.rgbv.z);
    c2 = dot(t, t);
    t = mk(a.nd.x, a.nd.y, a.nd.z) - mk(b.nd.x, b.nd.y, b.nd.z);
    const float dn = dot(t, t);
    n2 = dn > 0.0f ? dn : 0.0f;
    p2 = (a.nd.w - b.nd.w) * (a.nd.w - b.nd.w);
}

// c_w * n_w * p_w (left to right) of N pairs from their squared differences.
template <int N>
__device__ __forceinline__ void dn_dist_weights(const float c2[N], const float n2[N], const float p2[N], float out[N],
                                                const double* __restrict__ tab) {
    bool any_n = false, any_p = false;
#pragma unroll
    for (int i = 0; i < N; ++i) {
        any_n |= n2[i] != 0.0f;
        any_p |= p2[i] != 0.0f;
    }
    float cw[N], nw[N], pw[N];
    dn_weights<N>(c2, cw, tab);
    // a zero normal (depth) difference gives exactly 1 (dn_weight(0)); equal normals (the floor)
    // and the constant depth (a18) make whole batches of the wave skip the sequence
#pragma unroll
    for (int i = 0; i < N; ++i) nw[i] = pw[i] = 1.0f;
    if (__builtin_amdgcn_ballot_w64(any_n)) dn_weights<N>(n2, nw, tab);
    if (__builtin_amdgcn_ballot_w64(any_p)) dn_weights<N>(p2, pw, tab);
#pragma unroll
    for (int i = 0; i < N; ++i) out[i] = cw[i] * nw[i] * pw[i];
}

template <int N>
__device__ __forceinline__ void dn_pair_weights(const DnsPix a[N], const DnsPix& b, float out[N],
                                                const double* __restrict__ tab) {
    float c2[N], n2[N], p2[N];
#pragma unroll
    for (int i = 0; i < N; ++i) dn_pair_dist(a[i], b, c2[i], n2[i], p2[i]);
    dn_dist_weights<N>(c2, n2, p2, out, tab);
}

// Exhaustive check of the shipped weight (dn_weights: the short exp, the guard, the slow form's
// fallback and the 0 / >= 330 shortcuts) against dn_weight_slow (cpt_selftest_qdiv which = 6:
// mismatches over the float patterns [0, n); which = 7: how many of them take the fallback).
__global__ void k_selftest_dn_weight(int which, uint64_t n, unsigned long long* out, int out_len) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const float d = __uint_as_float((uint32_t)i);
        bool flag;
        if (which == 6) {
            float w;
            dn_weights<1>(&d, &w, g_dn_exp_table);
            const float w_ref = dn_weight_slow(d);
            flag = __float_as_uint(w) != __float_as_uint(w_ref);
        } else {
            const double e = dn_exp_short(d, g_dn_exp_table);
            flag = dn_near_midpoint(e) && !(d >= 330.0f);
        }
        if (flag) {
            unsigned long long k = atomicAdd(&out[0], 1ull);
            if ((long long)k + 1 < out_len) out[k + 1] = ((unsigned long long)__float_as_uint(d) << 32);
        }
    }
}

hipError_t launch_selftest_dn_weight(int which, uint64_t n, unsigned long long* out, int out_len, hipStream_t stream) {
    hipLaunchKernelGGL(k_selftest_dn_weight, dim3(8192), dim3(256), 0, stream, which, n, out, out_len);
    return hipGetLastError();
}

// The block's n waves (DNR_WAVES, 8) share the window: per super-step they take the next n
// rows, wave w row R = B + w:
//   1. each wave writes its row into the block's pixel ring (2n + 4 rows: the n new ones never
//      alias the n + 4 the other waves may still be reading for their taps);
//   barrier;
//   2. each wave computes its row's 12 pair weights into the block's weight ring (n + 2 rows),
//      then issues the loads of row R + n (the prefetch) and of its output row's mix;
//   barrier;
//   3. each wave finalizes output row O = R - 2 from the weights of rows O .. O + 2 and the pixel
//      rows O - 2 .. O + 2, in the reference's tap order, and stores it.
// Occupancy is the lever this kernel answered to (round 5, profiles/r05/ab_display_*.log, C4
// device frame): one wave per strip with its own 19.5 KB ring (k_denoise_strip, retired) 0.127 ms;
// 4-wave blocks sharing the rings, 3 waves per SIMD (150 VGPRs) 0.106-0.109; out-of-frame pairs
// stored as weight 0 so the taps need no branch (138 VGPRs) 0.097; 8-wave blocks at 4 waves per
// SIMD, batches of 4 pair weights and the loads issued after the pair weights (124 VGPRs, no
// spill) 0.090-0.092 (with the loads ahead of the pairs: 14 VGPRs spilled, 0.093-0.099).
// Those are round 5's registers.  Under the build's iterative-maxocc scheduler (build.py) and the
// current compiler every instantiation, HIST or not, has 128 VGPRs with 10 spilled to 28 B of
// scratch (profiles/r14/isa_compare.log), at the times of §11.3.
// Loads are issued unconditionally (out-of-frame lanes read a valid address and discard it)
// and the stores sit in a branch-free tail (lanes without an output pixel store to `sink`), so
// the next row's wait does not drain a branch's worth of stores.
// pixel ring: the n new rows + the 2n + 4 - n rows a slower wave may still read for its taps;
// weight ring: the n + 2 rows the taps of one super-step read
constexpr int DNR_WAVES = 8, DNR_PIX_ROWS = 2 * DNR_WAVES + 4, DNR_W_ROWS = DNR_WAVES + 2;
constexpr int DNR_MINWAVES = 4;        // __launch_bounds__ waves per SIMD (<= 128 VGPRs)
constexpr int DNR_BLOCKS_PER_CU = 2;   // 8-wave blocks, 4 waves per SIMD
constexpr int DN_BATCH = 4;            // pair weights evaluated together (a divisor of 12)
// the static LDS of one block: the exp table, the two pixel rings, the weight ring (78 KB)
constexpr size_t DNR_LDS_BYTES = DN_EXP_N * sizeof(double) + 2 * DNR_PIX_ROWS * DNS_LANES * sizeof(float4) +
                                 DNR_W_ROWS * 12 * DNS_LANES * sizeof(float);
static_assert(DNR_LDS_BYTES * DNR_BLOCKS_PER_CU <= 160 * 1024, "k_denoise_rows: blocks per CU exceed the CU's LDS");

// HIST (cpt_denoise_mix_history): Mix weighs each pixel by its own sample count n,
// read from `count` with the output row's mix and stored back as n + 1, in place of the frame's
// one 1 / cur_sample_idx: inv = 1 / (n + 1), the same correctly rounded quotient where n + 1 is
// that index.  Without it `count` is not read and the code is the kernel's as it was.
template <bool HOST, bool HIST>
__global__ void __launch_bounds__(DNS_LANES * DNR_WAVES, DNR_MINWAVES) k_denoise_rows(
    const float4* __restrict__ accum, const float* __restrict__ normal, const float* __restrict__ depth,
    float* __restrict__ mix, uint8_t* __restrict__ out, uint8_t* __restrict__ out_host, float4* __restrict__ sink,
    int width, int row0, int ctx_rows, int y0, int y1, int w_eff, int h_eff, int n_strips, int per_strip, float inv_idx,
    float* __restrict__ count) {
    __shared__ double s_tab[DN_EXP_N];
    __shared__ float4 rgbv[DNR_PIX_ROWS][DNS_LANES];
    __shared__ float4 ndr[DNR_PIX_ROWS][DNS_LANES];
    __shared__ float W[DNR_W_ROWS][12][DNS_LANES];
    for (int i = threadIdx.x; i < DN_EXP_N; i += DNS_LANES * DNR_WAVES) s_tab[i] = g_dn_exp_table[i];
    const int wv = (int)(threadIdx.x >> 6), j = (int)(threadIdx.x & 63);
    const int strip = (int)blockIdx.x % n_strips, part = (int)blockIdx.x / n_strips;
    const int nrow = y1 - y0;
    const int ra = y0 + (int)((long long)nrow * part / per_strip), rb = y0 + (int)((long long)nrow * (part + 1) / per_strip);
    const int c0 = strip * DNS_COLS;
    const int col = c0 - 2 + j;
    const int limit = w_eff * h_eff;
    const bool out_lane = j >= 2 && j < 2 + DNS_COLS && col < w_eff;
    float4* const sink_lane = sink + ((((uint32_t)blockIdx.x * DNR_WAVES + (uint32_t)wv) & 1023u) * 64u + (uint32_t)j);
    auto ring = [&](int row, int lane) {
        const int sl = (row + 4 * DNR_PIX_ROWS) % DNR_PIX_ROWS;
        return DnsPix{rgbv[sl][lane], ndr[sl][lane]};
    };
    auto cl = [](int l) { return l < 0 ? 0 : (l > 63 ? 63 : l); };
    auto load = [&](int Y, float4& a, float3& n, float& d, bool& valid) {
        const int L = Y * w_eff + col;
        valid = L >= 0 && L < limit;
        const int yy = col < 0 ? Y - 1 : (col >= w_eff ? Y + 1 : Y);
        const int xx = L - yy * w_eff;
        // the window reads up to a super-step past the rows it outputs; rows the context does not
        // hold (a band's, cpt_denoise_mix_band) are never a tap or pair of an output pixel, so
        // they read address 0 like the out-of-frame ones
        // (lanes past 2 W' of a narrow frame -- 16 or 32 columns -- wrap beyond the next row:
        // never a tap either, and outside the row they must not address)
        const bool held = yy - row0 >= 0 && yy - row0 < ctx_rows && xx >= 0 && xx < w_eff;
        const size_t px = valid && held ? (size_t)(yy - row0) * width + xx : (size_t)0;
        a = accum[px];
        n = make_float3(normal[3 * px], normal[3 * px + 1], normal[3 * px + 2]);
        d = depth[px];
    };
    auto put = [&](int Y, const float4& na, const float3& nn, float nd, bool nvalid) {
        const float4 a = nvalid ? na : make_float4(0.f, 0.f, 0.f, 0.f);
        const v3 c = a.w != 0.f ? mk(a.x, a.y, a.z) / a.w : mk(a.x, a.y, a.z);
        const int sl = (Y + 4 * DNR_PIX_ROWS) % DNR_PIX_ROWS;
        rgbv[sl][j] = make_float4(c.x, c.y, c.z, nvalid ? 1.f : 0.f);
        ndr[sl][j] = nvalid ? make_float4(nn.x, nn.y, nn.z, nd) : make_float4(0.f, 0.f, 0.f, 0.f);
    };
    constexpr float kernel5[5][5] = {{1.f, 4.f, 7.f, 4.f, 1.f},
                                     {4.f, 16.f, 26.f, 16.f, 4.f},
                                     {7.f, 26.f, 41.f, 26.f, 7.f},
                                     {4.f, 16.f, 26.f, 16.f, 4.f},
                                     {1.f, 4.f, 7.f, 4.f, 1.f}};
    // rows ra - 2 and ra - 1 (waves 0, 1): the pairs of rows ra, ra + 1 reach back into them
    float4 na;
    float3 nn;
    float nd;
    bool nvalid;
    if (wv < 2) {
        load(ra - 2 + wv, na, nn, nd, nvalid);
        put(ra - 2 + wv, na, nn, nd, nvalid);
    }
    load(ra + wv, na, nn, nd, nvalid);
#pragma unroll 1
    for (int B = ra; B - 2 < rb; B += DNR_WAVES) {
        const int R = B + wv;           // this wave's new row
        const int O = R - 2;            // the output row it finalizes
        float3 mix_cur;
        float cnt_cur = 0.f;
        auto load_mix = [&]() {
            const int orow = min(max(O, ra), rb - 1);
            const int ocol = min(max(col, 0), w_eff - 1);
            const size_t b = (size_t)(orow - y0) * width + ocol;
            mix_cur = make_float3(mix[3 * b], mix[3 * b + 1], mix[3 * b + 2]);
            if (HIST) cnt_cur = count[b];
        };
        put(R, na, nn, nd, nvalid);
        const DnsPix me = ring(R, j);   // (this lane's own write: ordered)
        __syncthreads();
        // ---- the 12 pair weights whose later pixel is (R, j) ---------------------------------------
        {
            float w12[12];
            // partner k of the 12 (k = 0, 1: (R, j + k + 1); 2..6: (R - 1, j + k - 4); 7..11:
            // (R - 2, j + k - 9)), in batches of DN_BATCH pairs
            auto partner = [&](int k) {
                return k < 2 ? ring(R, cl(j + k + 1)) : (k < 7 ? ring(R - 1, cl(j + k - 4)) : ring(R - 2, cl(j + k - 9)));
            };
#pragma unroll
            for (int k0 = 0; k0 < 12; k0 += DN_BATCH) {
                DnsPix a[DN_BATCH];
#pragma unroll
                for (int i = 0; i < DN_BATCH; ++i) a[i] = partner(k0 + i);
                dn_pair_weights<DN_BATCH>(a, me, w12 + k0, s_tab);
                // a pair with an out-of-frame pixel weighs +0 (the reference's c_w = n_w = p_w = 0),
                // so the taps need no branch: such a pixel's ring colour is +0 as well
#pragma unroll
                for (int i = 0; i < DN_BATCH; ++i)
                    w12[k0 + i] = a[i].rgbv.w != 0.f && me.rgbv.w != 0.f ? w12[k0 + i] : 0.f;
            }
            const int ws = (R + 4 * DNR_W_ROWS) % DNR_W_ROWS;
#pragma unroll
            for (int k = 0; k < 12; ++k) W[ws][k][j] = w12[k];
        }
        // the row a super-step ahead and the output row's mix, loaded after the pair weights (fewer
        // registers live through them)
        load(R + DNR_WAVES, na, nn, nd, nvalid);
        load_mix();
        __syncthreads();
        // ---- output row O (wave-uniform condition; every lane computes, out_lane stores) --------
        v3 st_m = mk1(0.f);
        uint32_t st_bgr = 0;
        bool st_real = false;
        if (O >= ra && O < rb) {
            const int wO = (O + 4 * DNR_W_ROWS) % DNR_W_ROWS, wO1 = (O + 1 + 4 * DNR_W_ROWS) % DNR_W_ROWS,
                      wO2 = (O + 2 + 4 * DNR_W_ROWS) % DNR_W_ROWS;
            const int jc = min(max(j, 2), 61);
            const DnsPix p = ring(O, jc);
            const bool finite = __builtin_isfinite(p.rgbv.x) && __builtin_isfinite(p.rgbv.y) &&
                                __builtin_isfinite(p.rgbv.z) && __builtin_isfinite(p.nd.x) &&
                                __builtin_isfinite(p.nd.y) && __builtin_isfinite(p.nd.z) && __builtin_isfinite(p.nd.w);
            float w_self = 1.0f;
            if (!finite) {
                float ws1[1];
                dn_pair_weights<1>(&p, p, ws1, s_tab);
                w_self = ws1[0];
            }
            v3 sum = mk1(0.f);
            float cum_w = 0.0f;
#pragma unroll
            for (int i = 0; i < 5; ++i) {
#pragma unroll
                for (int jj = 0; jj < 5; ++jj) {
                    const int u = i - 2, v = jj - 2;
                    const float4 q = rgbv[(O + v + 4 * DNR_PIX_ROWS) % DNR_PIX_ROWS][jc + u];
                    // (an out-of-frame q holds colour +0 and its pair weight +0: the reference's
                    // zero weight, without a branch)
                    const v3 ctmp = mk(q.x, q.y, q.z);
                    // where the pair (O, j) - (O + v, j + u) was stored: same row -- by the lane
                    // of its left pixel, as that pixel's forward pair |u| - 1; other rows -- by
                    // the lane of its lower pixel, at index 2 + dx + 2 (dy 1) or 7 + dx + 2
                    // (dy 2), dx = upper column - lower column
                    float weight;
                    if (u == 0 && v == 0) weight = w_self;
                    else if (v == 0 && u > 0) weight = W[wO][u - 1][jc];
                    else if (v == 0) weight = W[wO][-u - 1][jc + u];
                    else if (v < 0) weight = W[wO][v == -1 ? 2 + (u + 2) : 7 + (u + 2)][jc];
                    else weight = W[v == 1 ? wO1 : wO2][v == 1 ? 2 + (-u + 2) : 7 + (-u + 2)][jc + u];
                    sum = sum + (weight * kernel5[i][jj]) * ctmp;
                    cum_w += weight * kernel5[i][jj];
                }
            }
            const v3 dn = sum / cum_w;
            const v3 clp = mk(__builtin_fmaxf(0.f, __builtin_fminf(dn.x, 1.f)), __builtin_fmaxf(0.f, __builtin_fminf(dn.y, 1.f)),
                              __builtin_fmaxf(0.f, __builtin_fminf(dn.z, 1.f)));
            v3 m = mk(mix_cur.x, mix_cur.y, mix_cur.z);
            // (HIST: the weight is formed here, from the count, not held through the taps)
            m = m + (HIST ? 1.f / (cnt_cur + 1.f) : inv_idx) * (clp - m);   // lerp (helper_math.h:1154-1157)
            st_m = m;
            st_bgr = (uint32_t)(uint8_t)(255.99f * m.z) | ((uint32_t)(uint8_t)(255.99f * m.y) << 8) |
                     ((uint32_t)(uint8_t)(255.99f * m.x) << 16);
            st_real = out_lane;
        }
        {
            const size_t bself = st_real ? (size_t)(O - y0) * width + col : 0;
            float* const pm = st_real ? mix + 3 * bself : reinterpret_cast<float*>(sink_lane);
            uint32_t* const po = st_real ? reinterpret_cast<uint32_t*>(out) + bself : reinterpret_cast<uint32_t*>(sink_lane) + 3;
            pm[0] = st_m.x;
            pm[1] = st_m.y;
            pm[2] = st_m.z;
            *po = st_bgr;
            if (HIST) {
                float* const pc = st_real ? count + bself : reinterpret_cast<float*>(sink_lane);
                *pc = cnt_cur + 1.f;
            }
            if (HOST) {
                uint32_t* const ph = st_real ? reinterpret_cast<uint32_t*>(out_host) + bself : reinterpret_cast<uint32_t*>(sink_lane) + 3;
                *ph = st_bgr;
            }
        }
    }
}

// count != nullptr: the per-pixel Mix, which does not read cur_sample_idx.
hipError_t launch_denoise_mix(const float4* accum, const float* normal, const float* depth, float* mix, float* count,
                              uint8_t* out, uint8_t* out_host, float4* sink, int width, int height, int row0, int ctx_rows, int y0,
                              int y1, uint32_t cur_sample_idx, const LaunchGrid& grid, hipStream_t stream) {
    const int w_eff = 16 * (width / 16), h_eff = 16 * (height / 16);
    if (w_eff == 0 || h_eff == 0 || y1 <= y0) return hipSuccess;
    const int n_strips = (w_eff + DNS_COLS - 1) / DNS_COLS;
    const int rows = y1 - y0;
    int per_strip = (grid.cus * DNR_BLOCKS_PER_CU + n_strips - 1) / n_strips;
    per_strip = per_strip < 1 ? 1 : (per_strip > rows ? rows : per_strip);
    const unsigned blocks = (unsigned)(n_strips * per_strip);
    const float inv_idx = count ? 0.f : 1.f / float(cur_sample_idx);
    const dim3 grid_dim(blocks), block_dim(DNS_LANES * DNR_WAVES);
#define CPT_DN_LAUNCH(HOST, HIST)                                                                                             \
    hipLaunchKernelGGL((k_denoise_rows<HOST, HIST>), grid_dim, block_dim, 0, stream, accum, normal, depth, mix, out, out_host, \
                       sink, width, row0, ctx_rows, y0, y1, w_eff, h_eff, n_strips, per_strip, inv_idx, count)
    if (count) {
        if (out_host) CPT_DN_LAUNCH(true, true);
        else CPT_DN_LAUNCH(false, true);
    } else {
        if (out_host) CPT_DN_LAUNCH(true, false);
        else CPT_DN_LAUNCH(false, false);
    }
#undef CPT_DN_LAUNCH
    return hipGetLastError();
}

// The count plane's fill (a switch from cpt_denoise_mix to the per-pixel Mix): `value` in the
// first w_eff columns of `rows` rows of `width` floats.  One lane per float.
__global__ void __launch_bounds__(256) k_fill_count(float* __restrict__ count, int width, int w_eff, int rows, float value) {
    const int x = blockIdx.x * 256 + threadIdx.x;
    const int y = blockIdx.y;
    if (x < w_eff && y < rows) count[(size_t)y * width + x] = value;
}

hipError_t launch_fill_count(float* count, int width, int w_eff, int rows, float value, hipStream_t stream) {
    if (w_eff <= 0 || rows <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_fill_count, dim3((w_eff + 255) / 256, rows), dim3(256), 0, stream, count, width, w_eff, rows, value);
    return hipGetLastError();
}

// ======================================================================================
// Row-tile gather (cpt_gather_rows): a source context's rows, copied to this device as one
// block (accumulator float4s, then first-hit normals and depths), are scattered to the rows
// the destination frame holds them at.  One thread per pixel; every access is coalesced.
// ======================================================================================
__global__ void __launch_bounds__(256) k_stitch_rows(const float4* __restrict__ src_acc, const float* __restrict__ src_nrm,
                                                     const float* __restrict__ src_dep, const int32_t* __restrict__ dst_row,
                                                     int width, float4* __restrict__ acc, float* __restrict__ nrm,
                                                     float* __restrict__ dep) {
    const int x = blockIdx.x * blockDim.x + threadIdx.x;
    const int r = blockIdx.y;
    if (x >= width) return;
    const size_t s = (size_t)r * width + x, d = (size_t)dst_row[r] * width + x;
    acc[d] = src_acc[s];
    if (src_nrm) {
        nrm[3 * d] = src_nrm[3 * s];
        nrm[3 * d + 1] = src_nrm[3 * s + 1];
        nrm[3 * d + 2] = src_nrm[3 * s + 2];
        dep[d] = src_dep[s];
    }
}

hipError_t launch_stitch_rows(const float4* src_acc, const float* src_nrm, const float* src_dep, const int32_t* dst_row,
                              int width, int n_rows, float4* acc, float* nrm, float* dep, hipStream_t stream) {
    if (width <= 0 || n_rows <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_stitch_rows, dim3((width + 255) / 256, n_rows), dim3(256), 0, stream, src_acc, src_nrm, src_dep,
                       dst_row, width, acc, nrm, dep);
    return hipGetLastError();
}

// The adaptive moments of a source's rows (planar [4][src_npix]: m1, m2, k, rel) to the same
// destination rows of the destination's planes (planar [4][dst_npix]).  One lane per pixel, its
// four planes' words: each wave reads and writes 256 contiguous bytes per plane, and a lane's four
// loads are independent.
__global__ void __launch_bounds__(256) k_stitch_moments(const float* __restrict__ src, size_t src_npix,
                                                        const int32_t* __restrict__ dst_row, int width,
                                                        float* __restrict__ dst, size_t dst_npix) {
    const int x = blockIdx.x * blockDim.x + threadIdx.x;
    const int r = blockIdx.y;
    if (x >= width) return;
    const size_t s = (size_t)r * width + x, d = (size_t)dst_row[r] * width + x;
    const float m1 = src[s], m2 = src[src_npix + s], k = src[2 * src_npix + s], rel = src[3 * src_npix + s];
    dst[d] = m1;
    dst[dst_npix + d] = m2;
    dst[2 * dst_npix + d] = k;
    dst[3 * dst_npix + d] = rel;
}

hipError_t launch_stitch_moments(const float* src, size_t src_npix, const int32_t* dst_row, int width, int n_rows,
                                 float* dst, size_t dst_npix, hipStream_t stream) {
    if (width <= 0 || n_rows <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_stitch_moments, dim3((width + 255) / 256, n_rows), dim3(256), 0, stream, src, src_npix, dst_row,
                       width, dst, dst_npix);
    return hipGetLastError();
}
}  // namespace cpt
