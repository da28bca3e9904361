// Grouped and channel-view convolutions of fp32 engines on the matrix pipe for gfx950 (MI355X): the fp32 counterpart of conv_grouped.hip and conv_view.hip, a
// halo-patch convolution on v_mfma_f32_16x16x4_f32.  Activations, weights and sums are fp32; nothing is rounded to fp16.  These are the last convolutions an fp32
// engine ran on the scalar direct kernel: YOLOv9's DetectBbox_Conv (yolov9/src/block.cpp: 64 -> 64 with g = 4, 3x3 and 1x1) and the groups == 1 layers behind
// channel slices whose count, offset or stride is no multiple of 4 (RepNCSPELAN4 / RepNCSP at YOLOv9m's 90-channel widths), which conv_igemm_f32 declines.
//
// Scope (conv_patch_f32_supported): fp32 NHWC in / out / residual; stride 1, no dilation; 1x1 without padding or 3x3 with padding 1.
//   groups == 1: any Cin, any Cout, any channel offset and stride (base pointers 4-byte aligned);
//   2 <= groups <= 8: Cin / groups a multiple of 4 up to 64, Cout / groups a multiple of 16 up to 64, Cout <= 128, any channel offset and stride.
//
// Mapping (DESIGN.md "Grouped and view convolutions in fp32 engines"):
//   * persistent workgroups of 4 waves walk tiles of 4 x 16 output pixels (3x3; 1x1: 64 consecutive pixels of the N*H*W row).  A tile's work is a sequence of
//     ITEMS (column block, channel chunk): groups == 1 cuts the output channels into column blocks of at most 6 fragments of 16 and Cin into chunks of 32
//     (3x3) or 64 (1x1) channels; a grouped layer's column block is one group and its one chunk that group's input channels.  LDS holds two chunk patches
//     (at most 2 x 108 pixels x 68 floats = 57 KB, 31 KB for a groups == 1 3x3) whatever Cin is, so two to four workgroups share a CU;
//   * A operand: an item's halo patch (6 x 18 pixels; 1x1: 64) crosses L2 -> registers -> LDS once, not once per tap, as granules of 4 channels: one 16-byte
//     load where Cin, the channel stride and the base allow, four 4-byte loads otherwise (uniform per launch), one ds_write_b128 either way.  Every channel at
//     or beyond Cin and every pixel outside the image is WRITTEN as zero and never loaded: the neighbour channels of a view belong to another tensor and may
//     hold NaN.  The NEXT item's granules are loaded into registers before this item's k-loop and written to the other buffer after it: one barrier per item;
//   * LDS pixel pitch: 4 * ((chunk / 4) | 1) floats (36 for 32 channels, 68 for 64, 20 for 20): an odd number of 16-byte slots, so the 16 lanes of one k-slice
//     - 16 consecutive pixels, one ds_read_b128 each - start in 16 distinct 16-byte slots of the 256-byte bank row: no conflicts;
//   * B operand: packed fp32 weights straight from L2 with 16-byte loads one k-step ahead: groups == 1 the fp32 implicit-GEMM rows [Cout_pad][Kpad], tap-major,
//     CinK per tap (conv_layout_igemm_f32); grouped [group][Cout_g][Kpad], k = tap * Cin_g + c (conv_layout_grouped's rows in fp32);
//   * a k-step is 16 consecutive k of the item's K axis (tap-major over the chunk's channels; a lane's 4 never straddle a tap): one ds_read_b128 and one
//     16-byte weight load per fragment feed four v_mfma_f32_16x16x4_f32, MFMA e taking element e of every lane's four - the order conv_igemm_f32 sums a step
//     in.  The K order of a layer is chunk, tap, channel for every tile, column block and launch geometry: the same bits whatever the grid;
//   * waves: a block of one fragment (16 -> 16 per group) gives each wave one pixel fragment; wider blocks split 2 x 2, a wave owning two pixel fragments and
//     NH = ceil(fragments / 2) column fragments.  Accumulators stay in registers across a block's chunks;
//   * epilogue in registers, no LDS: a lane's fragment is four consecutive channels of one pixel: bias -> act1 -> (+ residual) -> act2 (act.h, the fp32
//     engines' family), one 16-byte store where the output view allows it, element-wise stores otherwise (uniform per launch; the residual likewise).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "../common.h"
#include "act.h"
#include "kernels.h"
#include "launch.h"

namespace trtx {
namespace {

constexpr int kTilePx = 64;        // 4 fragments of 16 pixels (3x3: 4 tile rows)
constexpr int kMaxFetch = 7;       // granules a lane holds of one patch: 108 pixels x 16 granules / 256 lanes
constexpr int kBlockFrags = 6;     // 16-channel output fragments of a column block, at most
constexpr int kMaxChunk = 64;      // channels of a patch, at most
constexpr int kLdsPerCu = 160 * 1024;

struct PfGeom {
    int tiles_x, tiles_y, total_tiles;
    int M;         // N * H * W
    int nblk;      // column blocks of a tile (grouped: the groups)
    int fpb;       // fragments of a block
    int frags;     // fragments of the layer
    int nchunk;    // channel chunks of a block (grouped: 1)
    int cw;        // channels of a full chunk (grouped: Cin per group)
    int cs;        // per-tap stride of a packed row (groups == 1: CinK; grouped: Cin per group)
    int pitch;     // floats per patch pixel
    int vec_in, vec_out, vec_res;   // 16-byte accesses on that side
};

struct PfTile {
    int n, ho0, wo0;
    long m0;
};

template <int TAPS>
__device__ __forceinline__ PfTile pf_decode(int tile, const PfGeom& g) {
    PfTile t{0, 0, 0, (long)tile * kTilePx};
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

// the channels an item reads: first channel inside the view, channels of the patch (a multiple of 4), first channel that is not the view's (or the group's)
__device__ __forceinline__ void pf_chunk(const ConvArgs& p, const PfGeom& g, int blk, int chunk, int* c0, int* cwc, int* cend) {
    if (p.groups > 1) {
        *c0 = blk * g.cw;
        *cwc = g.cw;
        *cend = *c0 + g.cw;
    } else {
        *c0 = chunk * g.cw;
        *cwc = min(g.cw, p.CinK - *c0);
        *cend = p.Cin;
    }
}

// an item's patch -> registers: consecutive lanes take consecutive granules of a pixel's channel row.  at[j]: the granule's place in a patch buffer (floats),
// ~0u for none.  Channels at or beyond cend and pixels outside the image stay zero and are written as such.
template <int TAPS>
__device__ __forceinline__ void pf_fetch(const ConvArgs& p, const PfGeom& g, int tile, int blk, int chunk, int tid, float4 (&v)[kMaxFetch], unsigned (&at)[kMaxFetch]) {
    constexpr int PW = TAPS == 9 ? 18 : 16, NPIX = (TAPS == 9 ? 6 : 4) * PW;
    int c0, cwc, cend;
    pf_chunk(p, g, blk, chunk, &c0, &cwc, &cend);
    const int gpp = cwc >> 2, total = NPIX * gpp;
    const float rgpp = 1.0f / (float)gpp;   // it < 1728 and gpp <= 16: (it + 0.5) / gpp is at least 1 / 32 away from an integer, the product below is exact enough
    const PfTile t = pf_decode<TAPS>(tile, g);
    const float* __restrict__ in = static_cast<const float*>(p.in);
#pragma unroll
    for (int j = 0; j < kMaxFetch; ++j) {
        const int it = j * 256 + tid;
        v[j] = make_float4(0.f, 0.f, 0.f, 0.f);
        at[j] = ~0u;
        if (it < total) {
            const int pp = (int)(((float)it + 0.5f) * rgpp), c = (it - pp * gpp) * 4;
            at[j] = (unsigned)(pp * g.pitch + c);
            long pix = -1;
            if (TAPS == 9) {
                const int py = pp / PW, px = pp - py * PW;
                const int hi = t.ho0 - 1 + py, wi = t.wo0 - 1 + px;
                if ((unsigned)hi < (unsigned)p.H && (unsigned)wi < (unsigned)p.W) pix = ((long)t.n * p.H + hi) * p.W + wi;
            } else if (t.m0 + pp < g.M) {
                pix = t.m0 + pp;
            }
            const int cg = c0 + c;
            if (pix >= 0 && cg < cend) {
                const float* src = in + pix * p.ld_in + cg;
                if (g.vec_in && cg + 4 <= cend) {
                    v[j] = *reinterpret_cast<const float4*>(src);
                } else {
                    v[j].x = src[0];
                    if (cg + 1 < cend) v[j].y = src[1];
                    if (cg + 2 < cend) v[j].z = src[2];
                    if (cg + 3 < cend) v[j].w = src[3];
                }
            }
        }
    }
}

__device__ __forceinline__ void pf_commit(float* buf, const float4 (&v)[kMaxFetch], const unsigned (&at)[kMaxFetch]) {
#pragma unroll
    for (int j = 0; j < kMaxFetch; ++j)
        if (at[j] != ~0u) *reinterpret_cast<float4*>(buf + at[j]) = v[j];
}

// TAPS: 1 (1x1) or 9 (3x3); PF: pixel fragments per wave (1: wave w owns fragment w and the block's one column fragment; 2: waves split 2 x 2);
// NH: column fragments per wave (1 .. 3)
template <int TAPS, int PF, int NH>
__global__ __launch_bounds__(256) void conv_patch_f32_kernel(const ConvArgs p, const PfGeom g) {
    constexpr int PW = TAPS == 9 ? 18 : 16, NPIX = (TAPS == 9 ? 6 : 4) * PW;
    extern __shared__ __attribute__((aligned(16))) float smem_f32[];

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int li = lane & 15, lj = lane >> 4;
    const int pf0 = PF == 2 ? 2 * (wave & 1) : wave;     // the wave's first pixel fragment
    const int cf0 = PF == 2 ? (wave >> 1) * NH : 0;      // ... and first column fragment inside a block
    const int buf_floats = NPIX * g.pitch;

    const float* __restrict__ wgt = static_cast<const float*>(p.wgt);
    const float* __restrict__ res = static_cast<const float*>(p.residual);
    float* __restrict__ out = static_cast<float*>(p.out);
    const bool second = res || p.act2 != ACT_NONE;

    float4 fv[kMaxFetch];
    unsigned fat[kMaxFetch];
    floatx4 acc[PF][NH];

    // ---- the first item's patch: nothing to hide it under
    int tile = blockIdx.x, blk = 0, chunk = 0;
    if (tile >= g.total_tiles) return;
    pf_fetch<TAPS>(p, g, tile, blk, chunk, tid, fv, fat);
    pf_commit(smem_f32, fv, fat);
    __syncthreads();

    int cur = 0;
    while (tile < g.total_tiles) {
        // ---- the next item (workgroup-uniform), its patch on the way while this one multiplies
        int ntile = tile, nblk = blk, nchunk = chunk + 1;
        if (nchunk == g.nchunk) {
            nchunk = 0;
            if (++nblk == g.nblk) {
                nblk = 0;
                ntile += gridDim.x;
            }
        }
        const bool more = ntile < g.total_tiles;
        if (more) pf_fetch<TAPS>(p, g, ntile, nblk, nchunk, tid, fv, fat);

        int c0, cwc, cend;
        pf_chunk(p, g, blk, chunk, &c0, &cwc, &cend);
        const int kend = TAPS * cwc, ksteps = (kend + 15) >> 4;
        const float rcw = 1.0f / (float)cwc;   // kk < 592, cwc <= 64: (kk + 0.5) / cwc is at least 1 / 128 away from an integer
        const int wk0 = p.groups > 1 ? 0 : c0;   // the chunk's first k inside a tap of the packed row

        const float* wrow[NH];
        bool flive[NH];   // wave-uniform
#pragma unroll
        for (int j = 0; j < NH; ++j) {
            const int cf = cf0 + j, cfa = blk * g.fpb + cf;
            flive[j] = cf < g.fpb && cfa < g.frags;
            wrow[j] = wgt + (size_t)((flive[j] ? cfa : 0) * 16 + li) * p.Kpad + wk0;   // (a dead fragment multiplies row 0 and is dropped)
        }
        if (chunk == 0) {
#pragma unroll
            for (int f = 0; f < PF; ++f)
#pragma unroll
                for (int j = 0; j < NH; ++j) acc[f][j] = floatx4{0.f, 0.f, 0.f, 0.f};
        }
        // the lane's 4 k of step ks: k = ks * 16 + 4 (lane >> 4) of the item's K axis = channels c .. c + 3 of tap k / cwc; beyond the axis: zeros on both sides
        const float* abase = smem_f32 + cur * buf_floats + (pf0 * PW + li) * g.pitch;
        auto kpos = [&](int ks, int* woff, int* aoff) {
            const int kk = ks * 16 + lj * 4;
            if (kk >= kend) return false;
            const int tap = TAPS == 1 ? 0 : (int)(((float)kk + 0.5f) * rcw);
            const int c = kk - tap * cwc;
            const int r = tap / 3, q = tap - 3 * r;
            *woff = tap * g.cs + c;
            *aoff = (TAPS == 9 ? r * PW + q : 0) * g.pitch + c;
            return true;
        };
        floatx4 b0[NH], b1[NH];
        int woff = 0, aoff = 0;
        bool klive = kpos(0, &woff, &aoff);
#pragma unroll
        for (int j = 0; j < NH; ++j) b0[j] = klive ? *reinterpret_cast<const floatx4*>(wrow[j] + woff) : floatx4{0.f, 0.f, 0.f, 0.f};
        for (int ks = 0; ks < ksteps; ++ks) {
            floatx4 a[PF];
#pragma unroll
            for (int f = 0; f < PF; ++f) a[f] = klive ? *reinterpret_cast<const floatx4*>(abase + f * PW * g.pitch + aoff) : floatx4{0.f, 0.f, 0.f, 0.f};
            klive = ks + 1 < ksteps && kpos(ks + 1, &woff, &aoff);
#pragma unroll
            for (int j = 0; j < NH; ++j) b1[j] = klive ? *reinterpret_cast<const floatx4*>(wrow[j] + woff) : floatx4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int e = 0; e < 4; ++e)
#pragma unroll
                for (int f = 0; f < PF; ++f)
#pragma unroll
                    for (int j = 0; j < NH; ++j) acc[f][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(b0[j][e], a[f][e], acc[f][j], 0, 0, 0);
#pragma unroll
            for (int j = 0; j < NH; ++j) b0[j] = b1[j];
        }
        if (more) pf_commit(smem_f32 + (cur ^ 1) * buf_floats, fv, fat);

        // ---- epilogue after a block's last chunk: the lane holds channels cb .. cb + 3 of pixel (lane & 15) of its fragments
        if (chunk == g.nchunk - 1) {
            const PfTile t = pf_decode<TAPS>(tile, g);
#pragma unroll
            for (int j = 0; j < NH; ++j) {
                if (!flive[j]) continue;
                const int cb = (blk * g.fpb + cf0 + j) * 16 + lj * 4;
                float b4[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) b4[e] = (p.bias && cb + e < p.Cout) ? p.bias[cb + e] : 0.f;
#pragma unroll
                for (int f = 0; f < PF; ++f) {
                    long m;
                    bool live;
                    if (TAPS == 9) {
                        const int ho = t.ho0 + pf0 + f, wo = t.wo0 + li;
                        live = ho < p.Ho && wo < p.Wo;
                        m = ((long)t.n * p.Ho + ho) * p.Wo + wo;
                    } else {
                        m = t.m0 + (pf0 + f) * 16 + li;
                        live = m < g.M;
                    }
                    if (!live || cb >= p.Cout) continue;
                    float v[4];
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[e] = act_f32(acc[f][j][e] + b4[e], p.act1, p.alpha1);
                    if (second) {
                        float r4[4] = {0.f, 0.f, 0.f, 0.f};
                        if (res) {
                            const float* rp = res + m * p.ld_res + cb;
                            if (g.vec_res) {
                                const float4 rv = *reinterpret_cast<const float4*>(rp);
                                r4[0] = rv.x; r4[1] = rv.y; r4[2] = rv.z; r4[3] = rv.w;
                            } else {
#pragma unroll
                                for (int e = 0; e < 4; ++e)
                                    if (cb + e < p.Cout) r4[e] = rp[e];
                            }
                        }
#pragma unroll
                        for (int e = 0; e < 4; ++e) v[e] = act_f32(v[e] + r4[e], p.act2, p.alpha2);
                    }
                    float* op = out + m * p.ld_out + cb;
                    if (g.vec_out) {
                        *reinterpret_cast<float4*>(op) = make_float4(v[0], v[1], v[2], v[3]);
                    } else {
#pragma unroll
                        for (int e = 0; e < 4; ++e)
                            if (cb + e < p.Cout) op[e] = v[e];
                    }
                }
            }
        }
        __syncthreads();   // the other buffer is written, this one is read: hand over
        cur ^= 1;
        tile = ntile;
        blk = nblk;
        chunk = nchunk;
    }
}

bool aligned_to(const void* p, uintptr_t n) { return (reinterpret_cast<uintptr_t>(p) & (n - 1)) == 0; }

// blocks, chunks and the patch pitch of a layer (a.CinK as conv_layout_patch_f32 leaves it)
void pf_split(const ConvArgs& a, PfGeom* g) {
    if (a.groups > 1) {
        g->nblk = a.groups;
        g->fpb = a.Cout / a.groups / 16;
        g->frags = g->nblk * g->fpb;
        g->nchunk = 1;
        g->cw = g->cs = a.Cin / a.groups;
    } else {
        g->frags = (a.Cout + 15) / 16;
        g->nblk = (g->frags + kBlockFrags - 1) / kBlockFrags;
        g->fpb = (g->frags + g->nblk - 1) / g->nblk;
        g->cs = a.CinK;
        g->cw = std::min(a.CinK, a.kh == 3 ? 32 : kMaxChunk);
        g->nchunk = (a.CinK + g->cw - 1) / g->cw;
    }
    g->pitch = 4 * ((g->cw / 4) | 1);
}

// The output may not lie on the input other than as another channel slice of the same map (a concat buffer): a workgroup stores its tile while others still
// read those pixels as halo.  Where both pointers are set.
bool output_on_input(const ConvArgs& a) {
    if (!a.in || !a.out) return false;
    const intptr_t pin = reinterpret_cast<intptr_t>(a.in), pout = reinterpret_cast<intptr_t>(a.out);
    const intptr_t in_bytes = (((intptr_t)a.N * a.H * a.W - 1) * a.ld_in + a.Cin) * 4;
    const intptr_t out_bytes = (((intptr_t)a.N * a.Ho * a.Wo - 1) * a.ld_out + a.Cout) * 4;
    if (pin + in_bytes <= pout || pout + out_bytes <= pin) return false;
    const intptr_t ld = (intptr_t)a.ld_in * 4;
    const bool out_behind = pout >= pin + (intptr_t)a.Cin * 4 && pout - pin + (intptr_t)a.Cout * 4 <= ld;
    const bool out_before = pin >= pout + (intptr_t)a.Cout * 4 && pin - pout + (intptr_t)a.Cin * 4 <= ld;
    return !(a.ld_in == a.ld_out && (out_behind || out_before));
}

template <int TAPS, int PF, int NH>
int32_t launch_patch_f32(const ConvArgs& a, const PfGeom& g, hipStream_t s) {
    const size_t lds = 2 * (size_t)(TAPS == 9 ? 6 * 18 : 64) * g.pitch * 4;   // at most 57.4 KB: below the 64 KB a kernel has without asking
    const int per_cu = std::max(2, std::min(4, (int)(kLdsPerCu / lds)));      // persistent workgroups: as many as the LDS keeps resident, on 256 CUs
    const int grid = std::min(g.total_tiles, 256 * per_cu);
    TRTX_LAUNCH((conv_patch_f32_kernel<TAPS, PF, NH>), dim3(grid), dim3(256), lds, s, a, g);
    return check_launch("conv_patch_f32");
}

}  // namespace

// plan time: pointers may be null (geometry only); launch time: the alignment of whatever pointers are set counts too
bool conv_patch_f32_supported(const ConvArgs& a) {
    if (!a.f32 || a.in_i8 || a.out_i8 || a.res_i8 || a.up_C != 0) return false;
    if (a.dil_h != 1 || a.dil_w != 1 || a.stride_h != 1 || a.stride_w != 1) return false;
    const bool k1 = a.kh == 1 && a.kw == 1 && a.pad_h == 0 && a.pad_w == 0;
    const bool k3 = a.kh == 3 && a.kw == 3 && a.pad_h == 1 && a.pad_w == 1;
    if (!k1 && !k3) return false;
    if (a.H <= 0 || a.W <= 0 || a.Ho != a.H || a.Wo != a.W) return false;   // (N is the enqueue's)
    if (a.Cin < 1 || a.Cout < 1 || a.ld_in < a.Cin || a.ld_out < a.Cout) return false;
    if ((a.residual || a.ld_res) && a.ld_res < a.Cout) return false;
    if (a.act1 < ACT_NONE || a.act1 > ACT_GELU_TANH || a.act2 < ACT_NONE || a.act2 > ACT_GELU_TANH) return false;
    if (a.groups == 1) {
        if (a.Cin > 4096) return false;   // (LDS holds one chunk at a time: the limit only keeps K in the ints of the packed row)
    } else {
        if (a.groups < 2 || a.groups > 8 || a.Cin % a.groups || a.Cout % a.groups) return false;
        const int cg = a.Cin / a.groups, og = a.Cout / a.groups;
        if (cg % 4 || cg > kMaxChunk || og % 16 || og > 64 || a.Cout > 128) return false;
    }
    if (!aligned_to(a.in, 4) || !aligned_to(a.out, 4) || !aligned_to(a.residual, 4)) return false;
    // tile counts and pixel indices are ints
    return (long)a.N * a.Ho * a.Wo < (1L << 30);
}

int32_t conv_patch_f32(const ConvArgs& a, hipStream_t s) {
    if (!a.in || !a.out || !a.wgt) return TRTX_ERR_INVALID;
    if (!conv_patch_f32_supported(a)) return TRTX_ERR_UNSUPPORTED;
    const int taps = a.kh * a.kw;
    if (a.groups == 1 ? (a.CinK != conv_igemm_f32_pick_cink(a.Cin) || a.Kpad != (taps * a.CinK + 15) / 16 * 16 || a.Cout_pad < (a.Cout + 15) / 16 * 16)
                      : a.Kpad != conv_grouped_kpad(a))
        return TRTX_ERR_UNSUPPORTED;
    if (!aligned_to(a.wgt, 16) || !aligned_to(a.bias, 4) || output_on_input(a)) return TRTX_ERR_INVALID;
    PfGeom g{};
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
    pf_split(a, &g);
    const int cg = a.Cin / a.groups;
    g.vec_in = cg % 4 == 0 && a.ld_in % 4 == 0 && aligned_to(a.in, 16);
    g.vec_out = a.Cout % 4 == 0 && a.ld_out % 4 == 0 && aligned_to(a.out, 16);
    g.vec_res = a.residual && a.Cout % 4 == 0 && a.ld_res % 4 == 0 && aligned_to(a.residual, 16);
    const int pf = g.fpb == 1 ? 1 : 2, nh = pf == 1 ? 1 : (g.fpb + 1) / 2;
#define PF_CASE(T, P, H) \
    if (taps == T && pf == P && nh == H) return launch_patch_f32<T, P, H>(a, g, s);
    PF_CASE(9, 1, 1) PF_CASE(9, 2, 1) PF_CASE(9, 2, 2) PF_CASE(9, 2, 3)
    PF_CASE(1, 1, 1) PF_CASE(1, 2, 1) PF_CASE(1, 2, 2) PF_CASE(1, 2, 3)
#undef PF_CASE
    return TRTX_ERR_UNSUPPORTED;
}

}  // namespace trtx
