// Convolution over channel views that are only 4-byte aligned, on the matrix pipe for gfx950 (MI355X): the groups == 1 layers that fell to the scalar
// direct kernel because the implicit-GEMM family reads its input in whole 16-byte pieces.  YOLOv9m's RepNCSPELAN4 stages have them (yolov9/src/block.cpp,
// RepNCSPELAN4 / RepNCSP / RepNBottleneck: inner widths 60 and 90, and the 180-channel halves of 360-channel tensors), and so has any user network
// whose ISliceLayer or concat lands on a channel count that is even but no multiple of 8.
//
// Scope (conv_view_supported): fp16 NHWC in / out / residual; groups == 1, no dilation, stride 1; 1x1 without padding or 3x3 with padding 1; Cin, Cout, every
// channel stride and (through the base pointers, which must be 4-byte aligned) every channel offset EVEN: the granule is 2 halves, one 4-byte load.
// 2 <= Cin <= kMaxCin = 256: two patch buffers of Cin rounded up to 32 channels (2 x 16 planes x 3456 B for a 3x3) plus the staging tile (13 KB) stay
// below the 160 KB of LDS a workgroup can have.  Any even Cout.
//
// Mapping (DESIGN.md "Convolutions over unaligned channel views"):
//   * persistent workgroups of 4 waves walk tiles of 4 x 16 output pixels (3x3; 1x1: 64 consecutive pixels of the N*H*W row).  A tile computes ALL output
//     channels, in column blocks of at most 6 fragments of 16 (Cout 60: one block of 4; 90: one of 6; 180: two of 6) over the one resident patch;
//   * A operand: the tile's halo patch (6 x 18 pixels; 1x1: 64) crosses HBM / L2 -> registers -> LDS ONCE, with 4-byte loads (8-byte loads where Cin, the
//     channel stride and the base allow: GR = 4), not once per filter tap.  Every granule at or beyond Cin and every pixel outside the image is written as
//     ZERO: the view's neighbour channels belong to another tensor, may hold NaN, and are never loaded.  The patch is laid out as conv_grouped.hip lays it
//     out: one plane per 16 channels, 32 bytes per pixel, so that the 16-lane groups of ds_read_b128 are bank-conflict free; the nine taps are nine offsets;
//   * the NEXT tile's patch is fetched under this tile's MFMAs into the second patch buffer: chunks of kFetch granules per lane are loaded at one k-step and
//     written to LDS two k-steps later (whatever is left after the last k-step follows the tile's stores);
//   * B operand: the implicit-GEMM family's packed weights as runtime/pack.cpp makes them ([Cout_pad][Kpad], tap-major, CinK = Cin rounded up to 32, zero
//     columns for the padding): always 16-byte aligned, streamed L2 -> registers with 16-byte loads two k-steps ahead;
//   * the four waves split a block 2 x 2: wave (pr, pc) owns pixel fragments 2 pr, 2 pr + 1 and NH = ceil(fragments / 2) column fragments: per k-step
//     2 ds_read_b128, NH 16-byte loads, 2 NH v_mfma_f32_16x16x32_f16.  K steps are tap-major, 32 channels each, and never straddle a tap;
//   * fp32 accumulation; epilogue bias -> act1 -> (+ residual) -> act2 in registers (act.h, the fast family), ONE fp16 rounding, then through an LDS staging
//     tile so that the stores are row-major pieces of 16, 8 or 4 bytes: the widest the output view allows, uniform per launch.
#include <hip/hip_fp16.h>
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <atomic>

#include "../common.h"
#include "act.h"
#include "kernels.h"
#include "launch.h"

namespace trtx {
namespace {

constexpr int kTilePx = 64;          // 4 fragments of 16 pixels (3x3: 4 tile rows)
constexpr int kMaxCin = 256;
constexpr int kBlockFrags = 6;       // 16-channel output fragments of a column block, at most
constexpr int kFetch = 8;            // granules a lane has in flight per fetch chunk
constexpr int kFetchLag = 2;         // k-steps between a chunk's loads and its LDS writes
constexpr int kLdsBudget = 160 * 1024;

struct VwGeom {
    int tiles_x, tiles_y, total_tiles;
    int M;        // N * H * W
    int spt;      // k-steps per tap: CinK / 32
    int frags;    // Cout rounded up to 16, in fragments
    int nblk;     // column blocks
    int fpb;      // fragments per block
    int vw;       // halves per store piece: 2, 4 or 8
    int nchunks;  // fetch chunks per patch
};

template <int GR> struct Gran;
template <> struct Gran<2> { typedef unsigned T; };
template <> struct Gran<4> { typedef uint2 T; };
__device__ __forceinline__ unsigned gran_zero(unsigned*) { return 0u; }
__device__ __forceinline__ uint2 gran_zero(uint2*) { return make_uint2(0u, 0u); }

struct VwTile {
    int n, ho0, wo0;
    long m0;
};

template <int TAPS>
__device__ __forceinline__ VwTile vw_decode(int tile, const VwGeom& g) {
    VwTile t{0, 0, 0, (long)tile * kTilePx};
    if (TAPS == 9) {
        const int tpi = g.tiles_x * g.tiles_y;
        t.n = tile / tpi;
        const int rem = tile - t.n * tpi;
        const int ty = rem / g.tiles_x;
        t.ho0 = ty * 4;
        t.wo0 = (rem - ty * g.tiles_x) * 16;
    }
    return t;
}

// one chunk of tile t's patch -> registers: consecutive lanes take consecutive granules of a pixel's channel row.  at[j]: the granule's place in a patch
// buffer, ~0u for none.  Granules at or beyond Cin and pixels outside the image stay zero and are written as such.
template <int TAPS, int GR>
__device__ __forceinline__ void vw_fetch_issue(const ConvArgs& p, const VwGeom& g, const VwTile& t, int chunk, int tid, typename Gran<GR>::T (&v)[kFetch],
                                               unsigned (&at)[kFetch]) {
    typedef typename Gran<GR>::T gran_t;
    constexpr int PW = TAPS == 9 ? 18 : 16, NPIX = (TAPS == 9 ? 6 : 4) * PW, PLANE = NPIX * 32;
    const int gpp = g.spt * (32 / GR), total = NPIX * gpp, live = p.Cin / GR;
    const _Float16* __restrict__ in = static_cast<const _Float16*>(p.in);
#pragma unroll
    for (int j = 0; j < kFetch; ++j) {
        const int it = (chunk * kFetch + j) * 256 + tid;
        v[j] = gran_zero(static_cast<gran_t*>(nullptr));
        at[j] = ~0u;
        if (it < total) {
            const int pp = it / gpp, gi = it - pp * gpp;
            const int c = gi * GR;
            at[j] = (unsigned)((c >> 4) * PLANE + pp * 32 + (c & 15) * 2);
            long pix = -1;
            if (TAPS == 9) {
                const int py = pp / PW, px = pp - py * PW;
                const int hi = t.ho0 - 1 + py, wi = t.wo0 - 1 + px;
                if ((unsigned)hi < (unsigned)p.H && (unsigned)wi < (unsigned)p.W) pix = ((long)t.n * p.H + hi) * p.W + wi;
            } else if (t.m0 + pp < g.M) {
                pix = t.m0 + pp;
            }
            if (gi < live && pix >= 0) v[j] = *reinterpret_cast<const gran_t*>(in + pix * p.ld_in + c);
        }
    }
}

template <int GR>
__device__ __forceinline__ void vw_fetch_commit(char* buf, const typename Gran<GR>::T (&v)[kFetch], const unsigned (&at)[kFetch]) {
#pragma unroll
    for (int j = 0; j < kFetch; ++j)
        if (at[j] != ~0u) *reinterpret_cast<typename Gran<GR>::T*>(buf + at[j]) = v[j];
}

// TAPS: 1 (1x1) or 9 (3x3); NH: column fragments per wave (1 .. 3); GR: halves per granule of the patch fetch (2 or 4)
template <int TAPS, int NH, int GR>
__global__ __launch_bounds__(256) void conv_view_f16_kernel(const ConvArgs p, const VwGeom g) {
    typedef typename Gran<GR>::T gran_t;
    constexpr int PW = TAPS == 9 ? 18 : 16, NPIX = (TAPS == 9 ? 6 : 4) * PW, PLANE = NPIX * 32;
    extern __shared__ __attribute__((aligned(16))) char smem[];

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int li = lane & 15, lj = lane >> 4;
    const int pr = wave & 1, pc = wave >> 1;
    const int patch_bytes = g.spt * 2 * PLANE;
    const int sp = g.fpb * 32 + 16;   // staging row pitch (bytes): 16 consecutive rows start in distinct 16-byte slots
    char* stage = smem + 2 * patch_bytes;
    const int KS = TAPS * g.spt;

    const _Float16* __restrict__ wgt = static_cast<const _Float16*>(p.wgt);
    const _Float16* __restrict__ res = static_cast<const _Float16*>(p.residual);
    _Float16* __restrict__ out = static_cast<_Float16*>(p.out);
    const bool second = res || p.act2 != ACT_NONE;

    gran_t fv[kFetch];
    unsigned fat[kFetch];

    // ---- the first tile's patch: nothing to hide it under
    int tile = blockIdx.x;
    VwTile t = vw_decode<TAPS>(tile, g);
    for (int ch = 0; ch < g.nchunks; ++ch) {
        vw_fetch_issue<TAPS, GR>(p, g, t, ch, tid, fv, fat);
        vw_fetch_commit<GR>(smem, fv, fat);
    }
    __syncthreads();

    int cur = 0;
    for (; tile < g.total_tiles; tile += gridDim.x) {
        const int nxt = tile + gridDim.x;
        const VwTile tn = vw_decode<TAPS>(nxt, g);
        const int fend = nxt < g.total_tiles ? g.nchunks : 0;   // chunks of the next tile's patch to fetch during this tile
        int fch = 0, step = 0, ready = 0;
        bool pending = false;
        const char* pa = smem + cur * patch_bytes;
        char* pb = smem + (cur ^ 1) * patch_bytes;
        // the lane's A address: pixel (lane & 15) of fragment 2 pr, chunk (lane >> 4) of a k-step's 32 channels (plane (lane >> 5), half (lane >> 4) & 1)
        const char* abase = pa + (lj >> 1) * PLANE + ((2 * pr) * PW + li) * 32 + (lj & 1) * 16;

        for (int blk = 0; blk < g.nblk; ++blk) {
            const int f0 = blk * g.fpb, fe = min(f0 + g.fpb, g.frags);
            const _Float16* wrow[NH];
            bool flive[NH];   // wave-uniform
#pragma unroll
            for (int j = 0; j < NH; ++j) {
                const int cf = f0 + pc * NH + j;
                flive[j] = pc * NH + j < g.fpb && cf < fe;
                wrow[j] = wgt + (size_t)((flive[j] ? cf : 0) * 16 + li) * p.Kpad + lj * 8;   // (a dead fragment multiplies row 0 and is dropped)
            }
            floatx4 acc[2][NH];
            half8 b0[NH], b1[NH], b2[NH];
#pragma unroll
            for (int j = 0; j < NH; ++j) {
                acc[0][j] = acc[1][j] = floatx4{0.f, 0.f, 0.f, 0.f};
                b0[j] = *reinterpret_cast<const half8*>(wrow[j]);
                b1[j] = *reinterpret_cast<const half8*>(wrow[j] + (KS > 1 ? 32 : 0));
            }
            int ks = 0;
#pragma unroll
            for (int tap = 0; tap < TAPS; ++tap) {
                const int toff = TAPS == 9 ? ((tap / 3) * PW + tap % 3) * 32 : 0;
                for (int s = 0; s < g.spt; ++s, ++ks, ++step) {
                    const int kn = ks + 2 < KS ? ks + 2 : KS - 1;
#pragma unroll
                    for (int j = 0; j < NH; ++j) b2[j] = *reinterpret_cast<const half8*>(wrow[j] + kn * 32);
                    // the next tile's patch, one chunk at a time (wave-uniform branches)
                    if (pending && step >= ready) {
                        vw_fetch_commit<GR>(pb, fv, fat);
                        pending = false;
                    }
                    if (!pending && fch < fend) {
                        vw_fetch_issue<TAPS, GR>(p, g, tn, fch++, tid, fv, fat);
                        pending = true;
                        ready = step + kFetchLag;
                    }
                    const char* ap = abase + toff + s * 2 * PLANE;
                    const half8 a0 = *reinterpret_cast<const half8*>(ap);
                    const half8 a1 = *reinterpret_cast<const half8*>(ap + PW * 32);
#pragma unroll
                    for (int j = 0; j < NH; ++j) {
                        acc[0][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(b0[j], a0, acc[0][j], 0, 0, 0);
                        acc[1][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(b0[j], a1, acc[1][j], 0, 0, 0);
                        b0[j] = b1[j];
                        b1[j] = b2[j];
                    }
                }
            }
            // ---- epilogue: the lane holds channels c0 .. c0 + 3 of pixel (lane & 15) of fragments 2 pr and 2 pr + 1
#pragma unroll
            for (int j = 0; j < NH; ++j) {
                if (!flive[j]) continue;
                const int c0 = (f0 + pc * NH + j) * 16 + lj * 4;
                const int lc0 = (pc * NH + j) * 16 + lj * 4;
                float b4[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) b4[e] = (p.bias && c0 + e < p.Cout) ? p.bias[c0 + e] : 0.f;
#pragma unroll
                for (int f2 = 0; f2 < 2; ++f2) {
                    const int f = 2 * pr + f2;
                    float v[4];
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[e] = act_fast(acc[f2][j][e] + b4[e], p.act1, p.alpha1);
                    if (second) {
                        float r4[4] = {0.f, 0.f, 0.f, 0.f};
                        if (res) {
                            long m;
                            bool live;
                            if (TAPS == 9) {
                                const int ho = t.ho0 + f, wo = t.wo0 + li;
                                live = ho < p.Ho && wo < p.Wo;
                                m = ((long)t.n * p.Ho + ho) * p.Wo + wo;
                            } else {
                                m = t.m0 + f * 16 + li;
                                live = m < g.M;
                            }
#pragma unroll
                            for (int h = 0; h < 2; ++h)   // Cout is even: a pair of channels is inside the view or outside it
                                if (live && c0 + 2 * h < p.Cout) {
                                    const __half2 rv = *reinterpret_cast<const __half2*>(res + m * p.ld_res + c0 + 2 * h);
                                    r4[2 * h] = __low2float(rv);
                                    r4[2 * h + 1] = __high2float(rv);
                                }
                        }
#pragma unroll
                        for (int e = 0; e < 4; ++e) v[e] = act_fast(v[e] + r4[e], p.act2, p.alpha2);
                    }
                    half4 o;
#pragma unroll
                    for (int e = 0; e < 4; ++e) o[e] = round_to_half(v[e]);
                    *reinterpret_cast<half4*>(stage + (f * 16 + li) * sp + lc0 * 2) = o;
                }
            }
            __syncthreads();

            // ---- staging -> global, row-major: consecutive lanes store consecutive pieces of a pixel's channel row
            const int bc0 = f0 * 16;
            const int cpo = (min(p.Cout - bc0, g.fpb * 16)) / g.vw;
            for (int it = tid; it < kTilePx * cpo; it += 256) {
                const int row = it / cpo, cc = it - row * cpo;
                long m;
                bool live;
                if (TAPS == 9) {
                    const int ho = t.ho0 + (row >> 4), wo = t.wo0 + (row & 15);
                    live = ho < p.Ho && wo < p.Wo;
                    m = ((long)t.n * p.Ho + ho) * p.Wo + wo;
                } else {
                    m = t.m0 + row;
                    live = m < g.M;
                }
                if (!live) continue;
                const char* src = stage + row * sp + cc * g.vw * 2;
                _Float16* dst = out + m * p.ld_out + bc0 + cc * g.vw;
                if (g.vw == 8)
                    *reinterpret_cast<half8*>(dst) = *reinterpret_cast<const half8*>(src);
                else if (g.vw == 4)
                    *reinterpret_cast<half4*>(dst) = *reinterpret_cast<const half4*>(src);
                else
                    *reinterpret_cast<unsigned*>(dst) = *reinterpret_cast<const unsigned*>(src);
            }
            __syncthreads();   // the staging tile is free for the next block / tile
        }
        // ---- what is left of the next patch (short K loops), then hand the buffers over
        while (pending || fch < fend) {
            if (pending) {
                vw_fetch_commit<GR>(pb, fv, fat);
                pending = false;
            }
            if (fch < fend) {
                vw_fetch_issue<TAPS, GR>(p, g, tn, fch++, tid, fv, fat);
                pending = true;
            }
        }
        __syncthreads();
        cur ^= 1;
        t = tn;
    }
}

int vw_cink(const ConvArgs& a) { return (a.Cin + 31) / 32 * 32; }
int vw_fpb(int frags) {
    const int nblk = (frags + kBlockFrags - 1) / kBlockFrags;
    return (frags + nblk - 1) / nblk;
}
size_t vw_lds_bytes(const ConvArgs& a) {
    const int npix = a.kh == 3 ? 6 * 18 : 64;
    return 2 * (size_t)(vw_cink(a) / 16) * npix * 32 + (size_t)kTilePx * (vw_fpb((a.Cout + 15) / 16) * 32 + 16);
}
bool aligned_to(const void* p, uintptr_t n) { return (reinterpret_cast<uintptr_t>(p) & (n - 1)) == 0; }

template <int TAPS, int NH, int GR>
int32_t launch_view(const ConvArgs& a, const VwGeom& g, hipStream_t s) {
    auto kern = conv_view_f16_kernel<TAPS, NH, GR>;
    static std::atomic<bool> attr_done[64];   // per instantiation and per device
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return TRTX_ERR_HIP;
    if (!attr_done[dev].load(std::memory_order_acquire)) {
        if (hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, kLdsBudget) != hipSuccess) {
            (void)hipGetLastError();
            return TRTX_ERR_HIP;
        }
        attr_done[dev].store(true, std::memory_order_release);
    }
    const size_t lds = vw_lds_bytes(a);
    const int per_cu = std::max(1, std::min(3, (int)(kLdsBudget / lds)));   // persistent workgroups: as many as the LDS keeps resident, on 256 CUs
    const int grid = std::min(g.total_tiles, 256 * per_cu);
    TRTX_LAUNCH(kern, dim3(grid), dim3(256), lds, s, a, g);
    return check_launch("conv_view_f16");
}

}  // namespace

bool conv_view_supported(const ConvArgs& a) {
    if (a.in_i8 || a.out_i8 || a.res_i8 || a.f32 || a.up_C != 0) return false;
    if (a.groups != 1 || a.dil_h != 1 || a.dil_w != 1 || a.stride_h != 1 || a.stride_w != 1) return false;
    const bool k1 = a.kh == 1 && a.kw == 1 && a.pad_h == 0 && a.pad_w == 0;
    const bool k3 = a.kh == 3 && a.kw == 3 && a.pad_h == 1 && a.pad_w == 1;
    if (!k1 && !k3) return false;
    if (a.H <= 0 || a.W <= 0 || a.Ho != a.H || a.Wo != a.W) return false;   // (N is the enqueue's)
    if (a.Cin < 2 || a.Cin > kMaxCin || a.Cin % 2 || a.ld_in % 2 || a.ld_in < a.Cin) return false;
    if (a.Cout < 2 || a.Cout % 2 || a.ld_out % 2 || a.ld_out < a.Cout) return false;
    if ((a.residual || a.ld_res) && (a.ld_res % 2 || a.ld_res < a.Cout)) return false;
    // whatever pointers are set: the channel offsets of the views are even
    if (!aligned_to(a.in, 4) || !aligned_to(a.out, 4) || !aligned_to(a.residual, 4)) return false;
    if (vw_lds_bytes(a) > (size_t)kLdsBudget) return false;
    // tile counts and pixel indices are ints
    return (long)a.N * a.Ho * a.Wo < (1L << 30);
}

int32_t conv_view(const ConvArgs& a, hipStream_t s) {
    if (!a.in || !a.out || !a.wgt) return TRTX_ERR_INVALID;
    const int taps = a.kh * a.kw, frags = (a.Cout + 15) / 16;
    if (!conv_view_supported(a) || a.CinK != vw_cink(a) || a.Kpad != taps * a.CinK || a.Cout_pad < frags * 16) return TRTX_ERR_UNSUPPORTED;
    if (!aligned_to(a.wgt, 16) || !aligned_to(a.bias, 4)) return TRTX_ERR_INVALID;
    VwGeom g{};
    g.M = a.N * a.Ho * a.Wo;
    if (g.M <= 0) return TRTX_OK;
    if (taps == 9) {
        g.tiles_x = (a.Wo + 15) / 16;
        g.tiles_y = (a.Ho + 3) / 4;
        g.total_tiles = a.N * g.tiles_x * g.tiles_y;
    } else {
        g.tiles_x = (g.M + kTilePx - 1) / kTilePx;
        g.tiles_y = 1;
        g.total_tiles = g.tiles_x;
    }
    g.spt = a.CinK / 32;
    g.frags = frags;
    g.nblk = (frags + kBlockFrags - 1) / kBlockFrags;
    g.fpb = vw_fpb(frags);
    // (the residual is read in 4-byte pairs whatever the piece)
    g.vw = (a.Cout % 8 == 0 && a.ld_out % 8 == 0 && aligned_to(a.out, 16)) ? 8 : ((a.Cout % 4 == 0 && a.ld_out % 4 == 0 && aligned_to(a.out, 8)) ? 4 : 2);
    const int gr = (a.Cin % 4 == 0 && a.ld_in % 4 == 0 && aligned_to(a.in, 8)) ? 4 : 2;
    const int npix = taps == 9 ? 6 * 18 : 64;
    g.nchunks = (npix * g.spt * (32 / gr) + 256 * kFetch - 1) / (256 * kFetch);
    const int nh = (g.fpb + 1) / 2;
#define VW_CASE(T, H, G) \
    if (taps == T && nh == H && gr == G) return launch_view<T, H, G>(a, g, s);
    VW_CASE(9, 1, 2) VW_CASE(9, 2, 2) VW_CASE(9, 3, 2) VW_CASE(9, 1, 4) VW_CASE(9, 2, 4) VW_CASE(9, 3, 4)
    VW_CASE(1, 1, 2) VW_CASE(1, 2, 2) VW_CASE(1, 3, 2) VW_CASE(1, 1, 4) VW_CASE(1, 2, 4) VW_CASE(1, 3, 4)
#undef VW_CASE
    return TRTX_ERR_UNSUPPORTED;
}

}  // namespace trtx
