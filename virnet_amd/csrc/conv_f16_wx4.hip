// conv_f16_wx4.hip -- the stride-1 3x3 convolution in Winograd F(4,3) form ALONG X (direct along y) on the CDNA4 f16 matrix pipe
// with SPLIT fp32 operands (gfx950).
//
// Same call sites as conv_f16.hip (AttResBlock.conv1/conv2, networks/AttResUNet.py:43,46,55,58; DnCNN mid convs, networks/DnCNN.py:25-28)
// and their input-gradient GEMMs.  Same arithmetic for every product (conv_f16.hip: v = hi + lo in fp16, three v_mfma_f32_32x32x16_f16
// per fp32 product, fp32 accumulation), but half of the products:
//
//   out[y][4t + k] = sum_j AT[k][j] * M_j[y][t],     M_j[y][t] = sum_dy sum_ci U[dy][j][co][ci] * V_j[y + dy - 1][t][ci]
//   U[dy][j] = sum_b G[j][b] w[dy][b]   (weights, transformed in fp64 when they are packed)
//   V_j[r][t] = sum_i BT[j][i] x[r][4t - 1 + i]   (6 input pixels -> 6 positions per 4-pixel x-tile, formed in fp32 while staging)
//
// i.e. 6 positions x 3 row taps = 18 MFMA k-steps per 4 output pixels instead of 36: 1.5 executed FLOP per algorithmic FLOP on the
// f16 pipe instead of 3.  Why 1-D and not F(2x2,3x3): the row taps accumulate into the SAME position accumulator, so a tile costs 6
// accumulators per 4 pixels (2-D F(2x2): 16 per 4) and a CU's register file holds a 16x32 pixel tile x 96 channels -- the transformed
// weights are then re-read from L2 once per 512 pixels (21 B/clk/CU at the pipe's peak; the 2-D form needs 43-85 B/clk/CU, more than the
// L2->LDS path delivers), and the input transform costs 1.8 VALU ops per MFMA instead of 3.6.  Numerics (tools/numerics_gate.py, whole
// denoise-syn network against fp64): 1.13e-5 max-abs on mu (fp32 direct 8.9e-6, 2-D F(2x2) 8.7e-6, 2-D F(4x4) 2.6e-5).
//
// Workgroup = 8 waves = one 16 x 32 pixel tile x 32*NREP output channels; wave (jt, rb) owns positions {3jt, 3jt+1, 3jt+2} of row
// block rb (4 rows x 8 x-tiles = the 32 columns of an MFMA): 3 x NREP accumulator blocks.  One workgroup per CU (LDS).
//   V (LDS, 54 KB): per position a hi and a lo plane of [18 rows][8 x-tiles] 32-byte records (16 fp16 channels), slot swizzle by row
//       parity -> conflict-free ds_read_b128 B fragments.  SINGLE buffered, replaced on the fly: a K chunk is walked as three stages
//       ji = 0,1,2 in which every wave works on position 3jt + ji, so planes {ji, 3+ji} are dead after stage ji and the threads write
//       the NEXT chunk's values into them during the following stage (raw pixels are held in registers across the three stages).
//   U (LDS, 2 x 12*NREP KB): stage = positions {ji, 3+ji} x 3 row taps x NREP slabs x (hi|lo) fragments of 1 KB, streamed by DMA
//       (buffer_load_dwordx4 ... lds: MUBUF, scalar piece offset) one stage ahead, double buffered; one barrier per stage (9*NREP MFMAs per wave).
//   Staging: thread = (V row 0..15, x-tile, channel quad): 6 pixels x 4 channels -> 6 positions x 4 channels; the tile's two halo rows
//       (V rows 16, 17) are 512 values per position pair = ONE extra scalar value per thread and stage.  All of it -- pixel loads,
//       pre-activation, rows of B^T, the exact hi/lo split, LDS stores, the DMA pieces, the fragment reads -- is cut into
//       micro-operations (the lambdas below) that tools/gen_wx4_sched.py places into the issue slots between the MFMAs of a stage
//       (conv_f16_wx4_sched.inc; every slot fenced with sched_barrier: hipcc's own scheduler clumps the VALU work and sinks the reads).
// Epilogue: the inverse transform crosses the two waves of a row block, so per 32-channel slab every wave writes three pre-combined
// blocks ([pixel][channel] records) to LDS and each thread finishes (pixel, channel quad) items from two or three of them: the same
// round trip also turns the tile around for 128-byte runs in the NHWC store.  Inverse scale, bias, mask, residual, activation as conv_f16.hip.
//
// WX4_X1 = 1 (set by conv_f16_wx4x1.hip, which includes this file for the kernel and its launcher only): the ONE-product form of the same
// kernel -- V and U carry the hi planes / pieces alone, the split's lo steps are gone and a stage is 3*NREP MFMAs (hi*hi), placed by the
// generator's --products 1 schedule.  Every difference is an `if constexpr (X1)` or a constant below; with WX4_X1 = 0 nothing changes.
#include "conv_f16_wx4_common.h"
#ifndef WX4_X1
#define WX4_X1 0
#endif
#if WX4_X1
#include "conv_f16_wx4x1_sched.inc"
#define conv_wx4_kernel conv_wx4x1_kernel
#define launch_wx4 launch_wx4x1
#else
#include "conv_f16_wx4_sched.inc"
#endif
#include <cstdlib>
#include <type_traits>

#ifndef WX4_LEDGER
#define WX4_LEDGER 0          // energy-ledger probe builds: see the stage lambda
#define WX4_LEDGER_OFF_
#endif
#ifndef WX4_STORE_AUX
#define WX4_STORE_AUX 0       // cache-policy bits of the epilogue's stores (probe builds: 1 sc0, 2 nt, 16 sc1)
#endif
#ifndef WX4_RES_AUX
#define WX4_RES_AUX 2         // ... of the epilogue's residual / mask tile loads: nt -- every byte is read exactly once (-0.7...1.0 % of J per conv2-type launch)
#endif
#ifndef WX4_LOAD_AUX
#define WX4_LOAD_AUX 0        // ... of the pixel loads
#endif
#ifndef WX4_LEDGER_TILEMOD
#define WX4_LEDGER_TILEMOD 4
#endif

namespace {
using namespace virnet;

constexpr int WX_PLANE = 18 * 8 * 32;        // one (position, hi|lo) plane: [18 rows][8 x-tiles][32 B]
constexpr bool X1 = WX4_X1 != 0;
constexpr int WX_POS = (X1 ? 1 : 2) * WX_PLANE;
constexpr int WX_UPIECES = X1 ? 6 : 12;      // 1-KB weight pieces of one stage and slab: [jt][dy]([hi|lo])
constexpr int WX_VBYTES = 6 * WX_POS;        // 55296
constexpr int WX_XBLK = 32 * 144 + 64;       // exchange block: [32 columns][32 channels + 16 B pad], skewed by 64 B against its neighbours
constexpr int WX_CHUNK_BYTES = 36 * 1024;
// one slab's weights of one 16-channel chunk: [6 positions][3 dy][hi|lo][1 KB] = WX_CHUNK_BYTES

// PRE: what the conv applies to x while it is staged -- 0: nothing; 1: lrelu(x, in_slope); 2: lrelu(x*in_mul+in_add, in_slope), the SFT
// pre-activation of AttResUNet.py:54-55 with per-(image, channel) vectors.
// TE = 1 (training step): the epilogue also emits the channel-major T image of the stored tensor and its channel sums (FArgs::t_out /
// t_col; conv_f16.hip has the same variant).  The epilogue reader's items become 8 CONSECUTIVE pixels of one row -- thread = (row of 16,
// x-segment of 4, channel quad) instead of (pixel column, row parity, channel quad) with row pairs as items -- so that a thread holds
// one 16-byte T unit per channel and plane and no second LDS pass is needed; every NHWC store still covers 128 contiguous bytes per 8 lanes.
template <int NREP, int EPI, int PRE, int TE = 0>
__global__ __launch_bounds__(512, 2) void conv_wx4_kernel(const FArgs a) {
  static_assert(!TE || EPI < 4, "T emission: single-store epilogues");
  static_assert(!TE || !X1, "T emission: the three-product kernel");
  constexpr int NB = 32 * NREP;
  constexpr int NDMA = WX_UPIECES * NREP;                  // 1-KB pieces of one weight stage: [jt][dy][slab][hi|lo]
  constexpr int USTAGE = NDMA * 1024;
  constexpr int NDI = (NDMA + 7) / 8;

  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* const v_lds = smem;
  char* const w_lds = smem + WX_VBYTES;
  constexpr int LDS_MAIN = WX_VBYTES + 2 * USTAGE > 24 * WX_XBLK ? WX_VBYTES + 2 * USTAGE : 24 * WX_XBLK;
  float* const sft_lds = reinterpret_cast<float*>(smem + LDS_MAIN) + 2 * NB;   // PRE 2: [in_mul | in_add] of the image's Cin channels
  float* const sb_lds = reinterpret_cast<float*>(smem + LDS_MAIN);   // [inverse scale | bias] of the NB channels: read back by the epilogue

  // ---- workgroup -> (tile, channel block): contiguous tile ranges per XCD (block b runs on XCD b%8), channel blocks adjacent
  const int ncb = a.NP / NB;
  const int xcd = blockIdx.x & 7;
  const int q = blockIdx.x >> 3;
  const int qt = fast_div(q, a.mg_ncb);             // (divisions by launch invariants through the host's magic numbers)
  const int cb = __builtin_amdgcn_readfirstlane(q - qt * ncb);
#if WX4_LEDGER & 64
  // ledger probe: every XCD walks the same WX4_LEDGER_TILEMOD tiles over and over -- the launch's activations stay in that XCD's L2
  // (4 tiles) or in the Infinity Cache (32): what HBM and the fabric cost is the difference to the plain build
  const int tile = __builtin_amdgcn_readfirstlane(xcd * a.tiles_per_xcd + qt % WX4_LEDGER_TILEMOD);
#else
  // (a.rev: the XCD walks its tile range backwards -- consecutive launches alternate, so a launch starts on the tiles its producer wrote last)
  const int tile = __builtin_amdgcn_readfirstlane(xcd * a.tiles_per_xcd + (a.rev ? a.tiles_per_xcd - 1 - qt : qt));
#endif
  if (qt >= a.tiles_per_xcd || tile >= a.ntiles) return;
  const int img = __builtin_amdgcn_readfirstlane(fast_div(tile, a.mg_tpi));
  const int trem = tile - img * (a.ntx * a.nty);
  const int ty = __builtin_amdgcn_readfirstlane(fast_div(trem, a.mg_ntx));
  const int tx = __builtin_amdgcn_readfirstlane(trem - ty * a.ntx);
  const int oy0 = ty * 16, ox0 = tx * 32;

  const int tid = threadIdx.x;
  TSTAMP(0);
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l31 = lane & 31, lhi = lane >> 5;
  const int lane16 = lane * 16;
  const int jt = wave & 1, rb = wave >> 1;
  const int nch = a.Cin >> 4;
  const float* const ximg = a.x + (size_t)img * a.H * a.W * a.Cin;
  // every pixel load goes through a buffer descriptor of this image: 32-bit offsets (vector: item + pixel, scalar: chunk), no 64-bit
  // address arithmetic
  const auto xrs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(ximg), 0, a.H * a.W * a.Cin * 4, 0x00020000);
  const int pxb = a.Cin * 4;                       // bytes per pixel

  // ---- staging.  Main item of a thread: (V row 0..15, x-tile, channel quad): 6 pixels x 4 channels -> 6 positions x 4 channels.
  // The tile's two halo rows (V rows 16, 17) are 2 x 8 x 16 x 6 values = 512 per position pair: ONE value per thread and stage.
  auto item_at = [&](int srow, int sxt, int chan, int dst) {
    WxItem it;
    const int gy = oy0 - 1 + srow, gx0 = ox0 - 1 + 4 * sxt;
    const bool rin = (unsigned)gy < (unsigned)a.H;
    it.inb = 0;
#pragma unroll
    for (int b = 0; b < 6; ++b) it.inb |= ((rin && (unsigned)(gx0 + b) < (unsigned)a.W) ? 1u : 0u) << b;
    it.voff = (unsigned)(((gy * a.W + gx0) * a.Cin + chan) * 4);
    it.dst = dst;
    return it;
  };
  const int sxt = (lane >> 2) & 7, sq = lane & 3, srow = tid >> 5;
  const WxItem it0 = item_at(srow, sxt, 4 * sq, (srow * 8 + sxt) * 32 + ((((sq >> 1) ^ (srow & 1))) << 4) + (sq & 1) * 8);
  // halo value of this thread: position jw + 3*hp of the pair being written, row 16 + (hg>>1), x-tile (hg&1)*4 + (lane>>4), channel lane&15
  const int hp = wave & 1, hg = wave >> 1, hch = lane & 15;
  const int hrow = 16 + (hg >> 1), hxt = (hg & 1) * 4 + (lane >> 4);
  const WxItem ith = item_at(hrow, hxt, hch, (hrow * 8 + hxt) * 32 + ((((hch >> 3) ^ (hrow & 1))) << 4) + (hch & 7) * 2);
  float hc[3][6];                                  // (wave-uniform) coefficients of the halo value per stage-pair
#pragma unroll
  for (int jw = 0; jw < 3; ++jw)
#pragma unroll
    for (int b = 0; b < 6; ++b)                      // (readfirstlane: keeps the 18 coefficients in scalar registers)
      hc[jw][b] = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, hp ? wx4_coef(jw + 3, b) : wx4_coef(jw, b))));
  char* const vh_lds = v_lds + hp * 3 * WX_POS;

  const float* const imul = PRE == 2 ? a.in_mul + (size_t)img * a.Cin : nullptr;
  const float* const iadd = PRE == 2 ? a.in_add + (size_t)img * a.Cin : nullptr;
  const float in_slope_eff = a.in_slope;
  f32x4 sm = f32x4{1.f, 1.f, 1.f, 1.f}, sa = f32x4{0.f, 0.f, 0.f, 0.f};     // SFT vectors of the chunk in d0 / dh (PRE == 2)
  float smh = 1.f, sah = 0.f;
  // ---- micro-operations of the staging work; tools/gen_wx4_sched.py places them into the issue slots between the MFMAs of a stage.
  // A pixel outside the image is requested at an offset beyond the descriptor's range: the load returns 0 (and lrelu(0) = 0: no mask;
  // with SFT vectors the mask is applied after the modulation).  The range check sees the vector offset alone, so the pixel's offset is
  // formed per load instead of riding in the scalar offset (an item whose FIRST pixel lies left of the image would wrap).
  f32x4 d0[6];
  float dh[6];
  int ld_so = 0;                                   // byte offset of the chunk whose pixels are being requested
  constexpr unsigned OOB = 0x80000000u;
  auto ldp = [&](auto bc) {
    constexpr int b = decltype(bc)::value;
    d0[b] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(xrs, ((it0.inb >> b) & 1u) ? it0.voff + b * pxb : OOB, ld_so, WX4_LOAD_AUX));
  };
  auto ldh = [&](auto bc) {
    constexpr int b = decltype(bc)::value;
    dh[b] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(xrs, ((ith.inb >> b) & 1u) ? ith.voff + b * pxb : OOB, ld_so, 0));
  };
  auto ldsft = [&]() {
    if constexpr (PRE == 2) {
      sm = *reinterpret_cast<const f32x4*>(imul + (ld_so >> 2) + 4 * sq);
      sa = *reinterpret_cast<const f32x4*>(iadd + (ld_so >> 2) + 4 * sq);
      smh = imul[(ld_so >> 2) + hch];
      sah = iadd[(ld_so >> 2) + hch];
    }
  };
  // K loop: the chunk's SFT vectors come from the LDS table the prologue filled -- read at the point of use (stage 1), so that no SFT
  // register is live across stages (the global-load form cost 14 spilled VGPRs at NREP 3: VERDICT r03 weak #7)
  auto rdsft = [&]() {
    if constexpr (PRE == 2) {
      // (the thread's offsets into the table are re-derived from lane16 -- live for the weight DMA anyway -- by two opaque VALU ops per
      // chunk: kept as loop invariants, the table addresses were parked in scratch and re-loaded INSIDE the K loop behind a vmcnt(0))
      int o4 = 0, o1 = 0;                                   // bytes: 4*sq*4 = lane16 & 48;  hch*4 = (lane16 >> 2) & 63
#if defined(__HIP_DEVICE_COMPILE__)
      asm volatile("v_and_b32 %0, 48, %1" : "=v"(o4) : "v"(lane16));
      asm volatile("v_bfe_u32 %0, %1, 2, 6" : "=v"(o1) : "v"(lane16));
#endif
      const char* const tb = reinterpret_cast<const char*>(sft_lds) + ld_so;
      sm = *reinterpret_cast<const f32x4*>(tb + o4);
      sa = *reinterpret_cast<const f32x4*>(tb + a.Cin * 4 + o4);
      smh = *reinterpret_cast<const float*>(tb + o1);
      sah = *reinterpret_cast<const float*>(tb + a.Cin * 4 + o1);
    }
  };
  // pre-activation (AttResUNet.py:54-55) of one loaded pixel quad: lrelu(x * mul + add), zero outside the image AFTER it
  auto pr = [&](auto bc) {
    constexpr int b = decltype(bc)::value;
    f32x4 x = d0[b];
    if constexpr (PRE == 2) x = x * sm + sa;
    const f32x4 t = x * in_slope_eff;
    f32x4 v = f32x4{vmax(x.x, t.x), vmax(x.y, t.y), vmax(x.z, t.z), vmax(x.w, t.w)};
    if constexpr (PRE == 2) v = ((it0.inb >> b) & 1u) ? v : f32x4{0.f, 0.f, 0.f, 0.f};
    d0[b] = v;
  };
  auto prH = [&](int b0) {
#pragma unroll
    for (int b = b0; b < b0 + 3; ++b) {
      float u = dh[b];
      if constexpr (PRE == 0) {
#if defined(__HIP_DEVICE_COMPILE__)
        asm volatile("" : "+v"(u));
#endif
      }
      if constexpr (PRE == 2) u = u * smh + sah;
      if constexpr (PRE >= 1) u = vmax(u, u * in_slope_eff);
      if constexpr (PRE == 2) u = ((ith.inb >> b) & 1u) ? u : 0.f;
      dh[b] = u;
    }
  };
  auto prHa = [&]() { prH(0); };
  auto prHb = [&]() { prH(3); };
  // one Winograd position of the main item: rows of B^T in two or three steps, exact fp16 split in three, one LDS store
  struct PutCtx { f32x4 a, b, v; unsigned h0, h1, l0, l1; };
  PutCtx pc[2];
  auto pA = [&](auto xc, auto jc) {
    constexpr int X = decltype(xc)::value, J = decltype(jc)::value;
    if constexpr (J == 0) pc[X].a = 4.f * d0[0] + d0[4];
    else if constexpr (J == 5) pc[X].a = 4.f * d0[1] + d0[5];
    else if constexpr (J == 1 || J == 2) pc[X].a = d0[4] - 4.f * d0[2];
    else pc[X].a = d0[4] - d0[2];
  };
  auto pB = [&](auto xc, auto jc) {
    constexpr int X = decltype(xc)::value, J = decltype(jc)::value;
    if constexpr (J == 1 || J == 2) pc[X].b = d0[3] - 4.f * d0[1];
    else pc[X].b = d0[3] - d0[1];
  };
  auto pV = [&](auto xc, auto jc) {
    constexpr int X = decltype(xc)::value, J = decltype(jc)::value;
    if constexpr (J == 0) pc[X].v = pc[X].a - 5.f * d0[2];
    else if constexpr (J == 5) pc[X].v = pc[X].a - 5.f * d0[3];
    else if constexpr (J == 1) pc[X].v = pc[X].a + pc[X].b;
    else if constexpr (J == 2) pc[X].v = pc[X].a - pc[X].b;
    else if constexpr (J == 3) pc[X].v = pc[X].a + 2.f * pc[X].b;
    else pc[X].v = pc[X].a - 2.f * pc[X].b;
  };
  float amax = 0.f;                                // range guard (conv_f16_common.h): largest transformed magnitude this thread staged
  auto pHi = [&](auto xc) {
    constexpr int X = decltype(xc)::value;
    amax = fmaxf(fmaxf(amax, fmaxf(fabsf(pc[X].v.x), fabsf(pc[X].v.y))), fmaxf(fabsf(pc[X].v.z), fabsf(pc[X].v.w)));
    pc[X].h0 = cvtpk(pc[X].v.x, pc[X].v.y);
    pc[X].h1 = cvtpk(pc[X].v.z, pc[X].v.w);
  };
  auto pSub = [&](auto xc) {
    constexpr int X = decltype(xc)::value;
    if constexpr (X1) return;
    pc[X].a = f32x4{subhi<0>(pc[X].v.x, pc[X].h0), subhi<1>(pc[X].v.y, pc[X].h0), subhi<0>(pc[X].v.z, pc[X].h1), subhi<1>(pc[X].v.w, pc[X].h1)};
  };
  auto pLo = [&](auto xc) {
    constexpr int X = decltype(xc)::value;
    if constexpr (X1) return;
    pc[X].l0 = cvtpk(pc[X].a.x, pc[X].a.y);
    pc[X].l1 = cvtpk(pc[X].a.z, pc[X].a.w);
  };
  // The V stores are written as asm: hipcc orders every LDS STORE it can see behind all pending weight pieces (an LDS-DMA piece is a
  // store to LDS for its wait-count pass: WAW), i.e. it puts s_waitcnt vmcnt(0) in front of the first store of every stage -- a wait for
  // the pieces just issued (and in stage 0 nothing else may be pending then).  The planes written here are dead planes of V, the pieces
  // go to U, and the end-of-stage wait covers lgkmcnt.
  const unsigned st_main = (unsigned)(size_t)(__attribute__((address_space(3))) char*)(v_lds + it0.dst);
  auto pSt = [&](auto xc, auto jc) {
    constexpr int X = decltype(xc)::value, J = decltype(jc)::value;
    const uint2 hi = make_uint2(pc[X].h0, pc[X].h1), lo = make_uint2(pc[X].l0, pc[X].l1);
    const unsigned ad = st_main;                     // (asm operands of a generic lambda must be its own locals)
    static_assert(WX_POS % 512 == 0 && WX_PLANE % 512 == 0, "ds_write2st64_b64 offsets are in units of 512 bytes");
    if constexpr (X1) asm volatile("ds_write_b64 %0, %1 offset:%2" ::"v"(ad), "v"(hi), "n"(J * WX_POS) : "memory");
    else asm volatile("ds_write2st64_b64 %0, %1, %2 offset0:%3 offset1:%4" ::"v"(ad), "v"(hi), "v"(lo), "n"(J * WX_POS / 512),
                 "n"((J * WX_POS + WX_PLANE) / 512)
                 : "memory");
  };
  // the thread's halo value of position pair JW
  float hv = 0.f, hw = 0.f;
  _Float16 hhi = (_Float16)0.f, hlo = (_Float16)0.f;
  auto hSa = [&](auto jwc) {
    constexpr int JW = decltype(jwc)::value;
    hv = fmaf(hc[JW][3], dh[3], fmaf(hc[JW][1], dh[1], hc[JW][0] * dh[0]));
  };
  auto hSb = [&](auto jwc) {
    constexpr int JW = decltype(jwc)::value;
    hw = fmaf(hc[JW][5], dh[5], fmaf(hc[JW][4], dh[4], hc[JW][2] * dh[2]));
  };
  auto hV = [&]() { hv += hw; };
  auto hHi = [&]() { amax = fmaxf(amax, fabsf(hv)); hhi = (_Float16)hv; };
  auto hSub = [&]() { if constexpr (!X1) hw = hv - (float)hhi; };
  auto hLo = [&]() { if constexpr (!X1) hlo = (_Float16)hw; };
  const unsigned st_halo = (unsigned)(size_t)(__attribute__((address_space(3))) char*)(vh_lds + ith.dst);
  auto hSt = [&](auto jwc) {
    constexpr int JW = decltype(jwc)::value;
    const unsigned h = __builtin_bit_cast(unsigned short, hhi), l = __builtin_bit_cast(unsigned short, hlo), ad = st_halo;
    if constexpr (X1) asm volatile("ds_write_b16 %0, %1 offset:%2" ::"v"(ad), "v"(h), "n"(JW * WX_POS) : "memory");
    else asm volatile("ds_write_b16 %0, %1 offset:%3\n\tds_write_b16 %0, %2 offset:%4" ::"v"(ad), "v"(h), "v"(l), "n"(JW * WX_POS),
                 "n"(JW * WX_POS + WX_PLANE)
                 : "memory");
  };
  // ---- weight DMA: piece q = i*8 + wave -> (jt, dy, slab, hi|lo) in LDS order; source = [slab][chunk][position][dy][hi|lo][1 KB].
  // Waves without a piece in the last round move their previous piece again (same bytes to the same place): no branch.
  const size_t slab_bytes = (size_t)nch * WX_CHUNK_BYTES;
  // (a buffer descriptor over this channel block's NREP slabs: the piece's source offset is scalar, the lane offset a constant register --
  // no per-piece 64-bit address arithmetic, and a MUBUF instruction, not a FLAT one)
  const auto wrs = __builtin_amdgcn_make_buffer_rsrc(const_cast<char*>(a.wimg + (size_t)(a.slab_base + cb * NREP) * slab_bytes), 0,
                                                     (int)(NREP * slab_bytes), 0x00020000);
  int poff[NDI], pdst[NDI];
#pragma unroll
  for (int i = 0; i < NDI; ++i) {
    int qd = i * 8 + wave;
    if (qd >= NDMA) qd -= 8;
    if constexpr (X1) { if (qd < 0) qd += NDMA; }      // (six pieces at NREP 1: waves 6 and 7 repeat pieces 4 and 5)
    if constexpr (X1) {                                 // hi pieces alone: (jt, dy, slab)
      const int jq = qd / (3 * NREP), r = qd - jq * (3 * NREP);
      const int dq = r / NREP, r2 = r - dq * NREP;
      poff[i] = __builtin_amdgcn_readfirstlane(r2 * (int)slab_bytes + jq * (3 * 3 * 2048) + dq * 2048);
    } else {
    const int jq = qd / (6 * NREP), r = qd - jq * (6 * NREP);
    const int dq = r / (2 * NREP), r2 = r - dq * (2 * NREP);
    poff[i] = __builtin_amdgcn_readfirstlane((r2 >> 1) * (int)slab_bytes + jq * (3 * 3 * 2048) + dq * 2048 + (r2 & 1) * 1024);
    }
    pdst[i] = __builtin_amdgcn_readfirstlane(qd * 1024);
  }
  (void)wrs; (void)lane16;                          // (only the device pass uses them: the builtin below is compiled out of the host pass)
  auto dma_piece = [&](int i, int src_off, char* wb) {      // src_off = chunk * 36 KB + ji * 6 KB
#if defined(__HIP_DEVICE_COMPILE__)                // (the host pass drops the kernel's stub without a diagnostic when it meets this builtin)
    __builtin_amdgcn_raw_ptr_buffer_load_lds(wrs, (__attribute__((address_space(3))) void*)(wb + pdst[i]), 16, lane16, src_off + poff[i], 0, 0);
#endif
  };

  // ---- fragment addressing
  int boff[3];
#pragma unroll
  for (int dy = 0; dy < 3; ++dy) {
    const int row = 4 * rb + dy + (l31 >> 3);
    boff[dy] = ((4 * rb + dy) * 8 + l31) * 32 + ((lhi ^ (row & 1)) << 4);
  }
  const int a_base = jt * (3 * NREP * (X1 ? 1024 : 2048)) + lane * 16;
  const char* const vjt = v_lds + jt * 3 * WX_POS;

  f32x16 acc[3][NREP];
#pragma unroll
  for (int j = 0; j < 3; ++j)
#pragma unroll
    for (int nr = 0; nr < NREP; ++nr)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[j][nr][r] = 0.f;

  // ---- prologue: weights of stage 0 by DMA; chunk 0's pixels -> positions {0,3} and {1,4} ({2,5} are written by stage 0 itself)
  const int nbase = a.slab_base * 32 + cb * NB;
  float sbv = 0.f;                                 // this thread's entry of the [inverse scale | bias] table
  if (tid < NB) sbv = a.inv_scale[nbase + tid];
  else if (tid < 2 * NB && a.bias) sbv = a.bias[nbase + tid - NB];
#ifdef WX4_PROBE_2X
  // probe build (profiles/r04_probes.md 4): prologue and plain epilogue executed a.nchw_op times -- what ONE prologue + epilogue pair
  // costs in launch time under the real power / memory conditions (the upper bound of what res-block fusion could delete)
  for (int prep = 0; prep < a.nchw_op; ++prep) {
  if (prep) { asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_barrier" ::: "memory"); }
#endif
#pragma unroll
  for (int i = 0; i < NDI; ++i) dma_piece(i, 0, w_lds);
#if WX4_LEDGER & 8
#pragma unroll
  for (int i = 0; i < NDI; ++i) dma_piece(i, 0, w_lds + USTAGE);       // ledger probe NODMA: both buffers hold stage 0 for good
#endif
  ldp(WX_I(0)); ldp(WX_I(1)); ldp(WX_I(2)); ldp(WX_I(3)); ldp(WX_I(4)); ldp(WX_I(5));
  ldh(WX_I(0)); ldh(WX_I(1)); ldh(WX_I(2)); ldh(WX_I(3)); ldh(WX_I(4)); ldh(WX_I(5));
  ldsft();
  if constexpr (PRE >= 1) {
    pr(WX_I(0)); pr(WX_I(1)); pr(WX_I(2)); pr(WX_I(3)); pr(WX_I(4)); pr(WX_I(5));
    prHa(); prHb();
  }
  pA(WX_I(0), WX_I(0)); pV(WX_I(0), WX_I(0)); pHi(WX_I(0)); pSub(WX_I(0)); pLo(WX_I(0)); pSt(WX_I(0), WX_I(0));
  pA(WX_I(1), WX_I(3)); pB(WX_I(1), WX_I(3)); pV(WX_I(1), WX_I(3)); pHi(WX_I(1)); pSub(WX_I(1)); pLo(WX_I(1)); pSt(WX_I(1), WX_I(3));
  pA(WX_I(0), WX_I(1)); pB(WX_I(0), WX_I(1)); pV(WX_I(0), WX_I(1)); pHi(WX_I(0)); pSub(WX_I(0)); pLo(WX_I(0)); pSt(WX_I(0), WX_I(1));
  pA(WX_I(1), WX_I(4)); pB(WX_I(1), WX_I(4)); pV(WX_I(1), WX_I(4)); pHi(WX_I(1)); pSub(WX_I(1)); pLo(WX_I(1)); pSt(WX_I(1), WX_I(4));
  hSa(WX_I(0)); hSb(WX_I(0)); hV(); hHi(); hSub(); hLo(); hSt(WX_I(0));
  hSa(WX_I(1)); hSb(WX_I(1)); hV(); hHi(); hSub(); hLo(); hSt(WX_I(1));
#if WX4_LEDGER & (16 | 256)
  // ledger probes NOSTAGE / NOVST: the K loop never writes V, so the prologue fills positions {2,5} as well
  pA(WX_I(0), WX_I(2)); pB(WX_I(0), WX_I(2)); pV(WX_I(0), WX_I(2)); pHi(WX_I(0)); pSub(WX_I(0)); pLo(WX_I(0)); pSt(WX_I(0), WX_I(2));
  pA(WX_I(1), WX_I(5)); pV(WX_I(1), WX_I(5)); pHi(WX_I(1)); pSub(WX_I(1)); pLo(WX_I(1)); pSt(WX_I(1), WX_I(5));
  hSa(WX_I(2)); hSb(WX_I(2)); hV(); hHi(); hSub(); hLo(); hSt(WX_I(2));
#endif
#ifdef WX4_PROBE_2X
  }
#endif
  if (tid < 2 * NB) sb_lds[tid] = sbv;
  if constexpr (PRE == 2) {
    for (int i = tid; i < a.Cin; i += 512) { sft_lds[i] = imul[i]; sft_lds[a.Cin + i] = iadd[i]; }
  }
  __syncthreads();
  TSTAMP(1);

  // One stage = positions {ji, 3+ji} of chunk c: 3*NREP groups (dy, slab) of three MFMAs into one accumulator block.  The body of a
  // stage is the generated issue schedule WX4_STAGE_<NREP>_<ji>_<PRE> (conv_f16_wx4_sched.inc): every MFMA sits behind a fenced slot
  // of fragment reads and micro-operations.  d0 / dh hold the pixels of the chunk whose V planes are being replaced:
  //   stage 0: positions {2,5} of chunk c (+ halo pair 2); then the pixels of chunk c+1 are requested into the freed registers
  //   stage 1: pre-activation of chunk c+1, positions {0,3};   stage 2: positions {1,4}    (planes {ji, 3+ji} die with stage ji)
  // The last chunk re-reads itself and rewrites its own dead planes: no branch in the stage code.  The end-of-stage wait of stage 0
  // leaves the pixel loads in flight: s_waitcnt vmcnt(pixel loads) covers the DMA pieces, which are issued before them.
  constexpr int NPX = 12;                           // VMEM instructions of one chunk's pixel loads (the SFT vectors come from LDS)
#if defined(VIRNET_F16_TIMING) && !defined(VIRNET_TIMING_LIGHT)      // (LIGHT: only the four TSTAMPs per workgroup -- the per-group stamps cost ~5 % of a tile)
  long long wx_tg[3][10] = {};
#endif
  // The stages of the LAST chunk (fin) have no next chunk to stage: stage 0 only finishes positions {2,5}, stages 1 and 2 read and
  // multiply, and stage 2 requests the epilogue's first operand tile (epf) into the registers the staging has released.
  constexpr int NIT = 8;                            // epilogue items of a thread: row pairs
  constexpr bool EPF = EPI == 1 || EPI == 2;        // ONE operand tile (residual or mask): prefetched slab by slab
  unsigned yoff[NIT];
  f32x4 op1[EPF ? NREP : 1][NIT];
  decltype(__builtin_amdgcn_make_buffer_rsrc((float*)nullptr, 0, 0, 0)) op1rs;
  auto epf = [&](auto ic) {
    constexpr int it = decltype(ic)::value;
    if constexpr (EPF) op1[0][it] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(op1rs, yoff[it], 0, WX4_RES_AUX));
  };
  auto stage = [&](int c, auto jic, auto finc) {
    constexpr int ji = decltype(jic)::value;
    constexpr bool fin = decltype(finc)::value;
    const int s = c * 3 + ji;
    const char* const wb = w_lds + (s & 1) * USTAGE + a_base;
    char* const wn = w_lds + ((s + 1) & 1) * USTAGE;
    const int cn = min(c + 1, nch - 1);
    // next stage's weights (the last stage fetches itself again into the idle buffer)
    const int src_off = ji < 2 ? c * WX_CHUNK_BYTES + (ji + 1) * 6144 : cn * WX_CHUNK_BYTES + (c + 1 < nch ? 0 : 2 * 6144);
    const char* const vb = vjt + ji * WX_POS;
    if constexpr (ji == 0) ld_so = cn * 64;
    h8 ah[3 * NREP], al[3 * NREP], bh[3], bl[3];
    // WX4_LEDGER (tools/probes/joule_ledger.py, profiles/r05_probes.md): probe builds that REMOVE one term of the stage each, so that the
    // launch's energy (socket W x ms) can be split by difference -- bit 1: no MFMA; 2: A fragments read once per stage (group 0 serves
    // all); 4: B fragments read once; 8: no weight DMA; 16: no staging arithmetic / V stores; 32: no pixel loads; 64: tiles stay in L2 /
    // the Infinity Cache (WX4_LEDGER_TILEMOD); 128: no epilogue; 256: staging arithmetic kept, V stores dropped; 512: epilogue without its
    // global stores; 1024 = the shipped code in a two-kernel build (base).  Never shipped.
    auto rdA = [&](auto gc) {
      constexpr int g = decltype(gc)::value;
      if constexpr ((WX4_LEDGER & 2) && g != 0) { ah[g] = ah[0]; al[g] = al[0]; return; }
      if constexpr (X1) { ah[g] = *reinterpret_cast<const h8*>(wb + g * 1024); return; }
      ah[g] = *reinterpret_cast<const h8*>(wb + (g * 2 + 0) * 1024);
      al[g] = *reinterpret_cast<const h8*>(wb + (g * 2 + 1) * 1024);
    };
    auto rdB = [&](auto dc) {
      constexpr int dy = decltype(dc)::value;
      if constexpr ((WX4_LEDGER & 4) && dy != 0) { bh[dy] = bh[0]; bl[dy] = bl[0]; return; }
      bh[dy] = *reinterpret_cast<const h8*>(vb + boff[dy]);
      if constexpr (!X1) bl[dy] = *reinterpret_cast<const h8*>(vb + WX_PLANE + boff[dy]);
    };
    auto dma = [&](auto ic) { if constexpr (!(WX4_LEDGER & 8)) dma_piece(decltype(ic)::value, src_off, wn); };
    auto mfma = [&](auto gc, auto pc_) {
      constexpr int g = decltype(gc)::value, part = decltype(pc_)::value;
      constexpr int dy = g / NREP, nr = g - dy * NREP;
      const h8 wa = part == 0 ? al[g] : ah[g];
      const h8 xv = part == 1 ? bl[dy] : bh[dy];
      if constexpr (WX4_LEDGER & 1) {
#if defined(__HIP_DEVICE_COMPILE__)
        asm volatile("" ::"v"(wa), "v"(xv));
#endif
      } else {
        acc[ji][nr] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wa, xv, acc[ji][nr], 0, 0, 0);
      }
    };
#if WX4_LEDGER & 16
    auto pA = [&](auto, auto) {}; auto pB = [&](auto, auto) {}; auto pV = [&](auto, auto) {};
    auto pHi = [&](auto) {}; auto pSub = [&](auto) {}; auto pLo = [&](auto) {}; auto pSt = [&](auto, auto) {};
    auto hSa = [&](auto) {}; auto hSb = [&](auto) {}; auto hV = [&]() {}; auto hHi = [&]() {}; auto hSub = [&]() {}; auto hLo = [&]() {};
    auto hSt = [&](auto) {}; auto pr = [&](auto) {}; auto prHa = [&]() {}; auto prHb = [&]() {}; auto rdsft = [&]() {};
#elif WX4_LEDGER & 256
    auto pSt = [&](auto xc, auto) {
      constexpr int X = decltype(xc)::value;
      const unsigned q0 = pc[X].h0, q1 = pc[X].h1, q2 = pc[X].l0, q3 = pc[X].l1;     // (asm operands of a generic lambda must be its own locals)
      (void)q0; (void)q1; (void)q2; (void)q3;
#if defined(__HIP_DEVICE_COMPILE__)
      asm volatile("" ::"v"(q0), "v"(q1), "v"(q2), "v"(q3));
#endif
    };
    auto hSt = [&](auto) {
      const unsigned h = __builtin_bit_cast(unsigned short, hhi), l = __builtin_bit_cast(unsigned short, hlo);
      (void)h; (void)l;
#if defined(__HIP_DEVICE_COMPILE__)
      asm volatile("" ::"v"(h), "v"(l));
#endif
    };
#endif
#if WX4_LEDGER & 32
    auto ldp = [&](auto) {}; auto ldh = [&](auto) {};
#endif
#if defined(VIRNET_F16_TIMING) && !defined(VIRNET_TIMING_LIGHT)      // (LIGHT: only the four TSTAMPs per workgroup -- the per-group stamps cost ~5 % of a tile)
    long long wx_tprev = (long long)__builtin_amdgcn_s_memtime();
#define WX_TS(g) do { const long long t_ = (long long)__builtin_amdgcn_s_memtime(); if ((g) < 9) wx_tg[ji][(g)] += t_ - wx_tprev; wx_tprev = t_; } while (0)
#else
#define WX_TS(g) do { } while (0)
#endif
#if WX4_X1
#define WX_STAGE_CASE(N_, J_, P_) if constexpr (!fin && NREP == N_ && ji == J_ && PRE == P_) { WX4X1_STAGE_##N_##_##J_##_##P_ }
#define WX_STAGE_FIN(N_, J_) if constexpr (fin && NREP == N_ && ji == J_) { WX4X1_FINAL_##N_##_##J_ }
#else
#define WX_STAGE_CASE(N_, J_, P_) if constexpr (!fin && NREP == N_ && ji == J_ && PRE == P_) { WX4_STAGE_##N_##_##J_##_##P_ }
#define WX_STAGE_FIN(N_, J_) if constexpr (fin && NREP == N_ && ji == J_) { WX4_FINAL_##N_##_##J_ }
#endif
#define WX_STAGE_PRE(N_, J_) WX_STAGE_CASE(N_, J_, 0) WX_STAGE_CASE(N_, J_, 1) WX_STAGE_CASE(N_, J_, 2) WX_STAGE_FIN(N_, J_)
    WX_STAGE_PRE(1, 0) WX_STAGE_PRE(1, 1) WX_STAGE_PRE(1, 2)
    WX_STAGE_PRE(2, 0) WX_STAGE_PRE(2, 1) WX_STAGE_PRE(2, 2)
    WX_STAGE_PRE(3, 0) WX_STAGE_PRE(3, 1) WX_STAGE_PRE(3, 2)
#undef WX_STAGE_PRE
#undef WX_STAGE_FIN
#undef WX_STAGE_CASE
    // end of stage: this wave's DMA pieces have landed (they are older than the pixel loads of stage 0, which stay in flight), its
    // LDS writes are done; then the workgroup barrier
    // The waits are the BUILTIN, which hipcc's wait-count pass can see (an asm one is opaque to it): a weight piece is a FLAT
    // instruction that writes LDS, and while the compiler believes one is pending it turns every wait it inserts into vmcnt(0).
    // Stage 0 leaves its NPX pixel loads in flight (the pieces are older); the last chunk has none, and its stage 2 issued no piece
    // but requested the epilogue's operand tile, which stays in flight.
#if (WX4_LEDGER & 16) && !(WX4_LEDGER & 32) && defined(__HIP_DEVICE_COMPILE__)
    if constexpr (ji == 1 && !fin) {                                           // ledger NOSTAGE: the pixel loads stay, their values are dropped here
#pragma unroll
      for (int b = 0; b < 6; ++b) asm volatile("" ::"v"(d0[b]), "v"(dh[b]));
    }
#endif
    constexpr int WAIT_ALL = 0x0070;                                           // vmcnt(0) expcnt(7) lgkmcnt(0)
    constexpr int WAIT_PX = (NPX & 15) | 0x0070 | ((NPX >> 4) << 14);          // vmcnt(NPX) lgkmcnt(0)
    constexpr int WAIT_LDS = 0xC07F;                                           // lgkmcnt(0) only
    if constexpr (ji == 0 && !fin) __builtin_amdgcn_s_waitcnt(WAIT_PX);
    else if constexpr (ji == 2 && fin) __builtin_amdgcn_s_waitcnt(WAIT_LDS);
    else __builtin_amdgcn_s_waitcnt(WAIT_ALL);
    asm volatile("s_barrier" ::: "memory");
#if defined(VIRNET_F16_TIMING) && !defined(VIRNET_TIMING_LIGHT)      // (LIGHT: only the four TSTAMPs per workgroup -- the per-group stamps cost ~5 % of a tile)
    wx_tg[ji][9] += (long long)__builtin_amdgcn_s_memtime() - wx_tprev;       // tail slot + waits + barrier
#endif
#undef WX_TS
  };
  using No = std::false_type;
  using Yes = std::true_type;
  for (int c = 0; c + 1 < nch; ++c) {
    stage(c, WX_I(0), No{});
    stage(c, WX_I(1), No{});
    stage(c, WX_I(2), No{});
  }
  stage(nch - 1, WX_I(0), Yes{});
  stage(nch - 1, WX_I(1), Yes{});
  // epilogue reader: thread = (pixel column x of the tile, channel quad cq), items it = row pairs.  One 32-bit byte offset per item
  // serves the operand loads and the stores (buffer instructions; an item outside the image gets an out-of-range offset: loads 0,
  // stores nothing).
  // The epilogue's thread coordinates are re-derived HERE from the wave index (a scalar) and the lane count, through an opaque copy:
  // derived from `tid` they stay live across the whole K loop, and at the 256-register budget the PRE 2 instantiations parked 3-7 of
  // them in scratch around the loop.
  int tid_e = wave * 64 + (int)__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
#if defined(__HIP_DEVICE_COMPILE__)
  asm volatile("" : "+v"(tid_e));
#endif
  const int lane_e = tid_e & 63, l31_e = lane_e & 31, lhi_e = lane_e >> 5;
  const int cq = tid_e & 7, px = (tid_e >> 3) & 31, prow = tid_e >> 8;
  const int te_row = tid_e >> 5, te_xq = (tid_e >> 3) & 3;       // TE mapping: tile row 0..15, x-segment 0..3 (items = its 8 pixels)
  const int C = a.cout;
  const size_t img_off = (size_t)img * a.H * a.W * C;
#pragma unroll
  for (int it = 0; it < NIT; ++it) {
    const int oy = TE ? oy0 + te_row : oy0 + 2 * it + prow, ox = TE ? ox0 + te_xq * 8 + it : ox0 + px;
    yoff[it] = (oy < a.H && ox < a.W) ? (unsigned)((oy * a.W + ox) * C + nbase + cq * 4) * 4u : 0x80000000u;
  }
  if constexpr (EPF) op1rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>((EPI == 1 ? a.res : a.mask) + img_off), 0, a.H * a.W * C * 4, 0x00020000);
  stage(nch - 1, WX_I(2), Yes{});
  TSTAMP(2);
  range_report(a.range_flag, amax);
#if (WX4_LEDGER & (1 | 128)) && defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
  for (int j = 0; j < 3; ++j)
#pragma unroll
    for (int nr = 0; nr < NREP; ++nr) asm volatile("" : "+v"(acc[j][nr]));     // ledger probes: the accumulators stay opaque / alive
#endif
#if WX4_LEDGER & 128
  return;
#endif
#if defined(VIRNET_F16_TIMING) && !defined(VIRNET_TIMING_LIGHT)      // (LIGHT: only the four TSTAMPs per workgroup -- the per-group stamps cost ~5 % of a tile)
  if (a.tlog && (tid & 63) == 0) {
#pragma unroll
    for (int j = 0; j < 3; ++j)
#pragma unroll
      for (int g = 0; g < 10; ++g) a.tlog[(size_t)a.ntiles * ncb * 8 + ((size_t)blockIdx.x * 8 + wave) * 32 + j * 10 + g] = wx_tg[j][g];
  }
#endif

  // ---- epilogue.  Per slab: wave (jt, rb) writes three blocks of [column = (row, x-tile)][32 channels] records
  //   jt = 0: A0 = M0+M1+M2, A1 = M1-M2, A2 = M1+M2        jt = 1: S = M3+M4, D = M3-M4, E = M5
  // and pixel k of an x-tile is  k=0: A0 + S   k=1: A1 + 2D   k=2: A2 + 4S   k=3: A1 + 8D + E   (rows of AT).
  char* const xb = smem;
  const int wblk = (rb * 6 + jt * 3) * WX_XBLK + l31_e * 144 + lhi_e * 16;
  auto put_block = [&](int which, const f32x16& m) {
#pragma unroll
    for (int g = 0; g < 4; ++g)
      *reinterpret_cast<f32x4*>(xb + wblk + which * WX_XBLK + g * 32) = f32x4{m[4 * g], m[4 * g + 1], m[4 * g + 2], m[4 * g + 3]};
  };
  auto xwrite = [&](int nr) {
    f32x16 b0, b1, b2;
    if (jt == 0) {
      b2 = acc[1][nr] + acc[2][nr];
      b1 = acc[1][nr] - acc[2][nr];
      b0 = acc[0][nr] + b2;
    } else {
      b0 = acc[0][nr] + acc[1][nr];
      b1 = acc[0][nr] - acc[1][nr];
      b2 = acc[2][nr];
    }
    put_block(0, b0); put_block(1, b1); put_block(2, b2);
  };
  const int pk = px & 3, pxt = px >> 2;
  const int r_p = ((pk == 0) ? 0 : (pk == 2) ? 2 : 1) * WX_XBLK + pxt * 144 + cq * 16;
  const int r_q = (3 + (pk & 1)) * WX_XBLK + pxt * 144 + cq * 16;
  const int r_e = 5 * WX_XBLK + pxt * 144 + cq * 16;
  const float ck = (float)(1 << pk), ek = pk == 3 ? 1.f : 0.f;
  const int te_base = (te_row >> 2) * 6 * WX_XBLK + ((te_row & 3) * 8) * 144 + cq * 16;   // TE: the thread's row (row block, row in block)
  auto xread = [&](int it) {                                // row = 2*it + prow: row block it>>1, row-in-block (it&1)*2 + prow
    if constexpr (TE) {                                     // pixel te_xq*8 + it of row te_row: x-tile te_xq*2 + (it>>2), pixel-in-tile it&3
      const int pkk = it & 3;
      const int b0 = te_base + (te_xq * 2 + (it >> 2)) * 144;
      const f32x4 p = *reinterpret_cast<const f32x4*>(xb + b0 + ((pkk == 0) ? 0 : (pkk == 2) ? 2 : 1) * WX_XBLK);
      const f32x4 qv = *reinterpret_cast<const f32x4*>(xb + b0 + (3 + (pkk & 1)) * WX_XBLK);
      f32x4 r = p + (float)(1 << pkk) * qv;
      if (pkk == 3) r += *reinterpret_cast<const f32x4*>(xb + b0 + 5 * WX_XBLK);
      return r;
    }
    const int base = (it >> 1) * 6 * WX_XBLK + (((it & 1) * 2 + prow) * 8) * 144;
    const f32x4 p = *reinterpret_cast<const f32x4*>(xb + base + r_p);
    const f32x4 qv = *reinterpret_cast<const f32x4*>(xb + base + r_q);
    const f32x4 e = *reinterpret_cast<const f32x4*>(xb + base + r_e);
    return p + ck * qv + ek * e;
  };
  const f32x4 zero4 = f32x4{0.f, 0.f, 0.f, 0.f};
  auto mask4 = [&](f32x4 v, f32x4 m) {
    return f32x4{m.x > 0.f ? v.x : v.x * a.mask_slope, m.y > 0.f ? v.y : v.y * a.mask_slope,
                 m.z > 0.f ? v.z : v.z * a.mask_slope, m.w > 0.f ? v.w : v.w * a.mask_slope};
  };
  // inverse scale / bias of the thread's channel quad: from the table the prologue left in LDS (no global load in the epilogue's way)
  auto inv_of = [&](int nr) { return *reinterpret_cast<const f32x4*>(sb_lds + nr * 32 + cq * 4); };
  auto bias_of = [&](int nr) { return *reinterpret_cast<const f32x4*>(sb_lds + NB + nr * 32 + cq * 4); };
  if constexpr (EPI < 4) {
    // ONE stored tensor.  gfx950 counts loads and stores on one vmcnt that must be treated as out of order once both kinds are
    // pending (conv_f16.hip), so a load consumed while stores are pending costs vmcnt(0).  With ONE operand tile (residual or mask; EPF)
    // slab 0's tile was requested in the K loop's last stage, slab 1's follows the first exchange write (its accumulators are free
    // then) and slab nr+2's goes out in front of slab nr's stores: the vmcnt(0) happens once, in slab 1, when everything outstanding is
    // a whole exchange phase old.  EPI 3 (mask AND residual) cannot hold the tiles and loads per slab.
    constexpr bool RES = (EPI & 1) != 0, MASK = (EPI & 2) != 0;
    float* const y = (a.y_act ? a.y_act : a.y_raw) + img_off;
    const float slope_eff = a.y_act ? a.slope : 1.f;
    auto load_op1 = [&](int nr) {
#pragma unroll
      for (int it = 0; it < NIT; ++it)
        op1[EPF ? nr : 0][it] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(op1rs, yoff[it] + nr * 128, 0, WX4_RES_AUX));
    };
    const auto yrs = __builtin_amdgcn_make_buffer_rsrc(y, 0, a.H * a.W * C * 4, 0x00020000);
#ifdef WX4_PROBE_2X
    for (int erep = 0; erep < (EPI == 0 ? a.nchw_op : 1); ++erep) {
    if (erep) wx_lds_barrier();
#endif
    xwrite(0);
    if (EPF && NREP > 1) load_op1(1);
#pragma unroll
    for (int nr = 0; nr < NREP; ++nr) {
      if (nr > 0) xwrite(nr);
      wx_lds_barrier();
      if (nr == 0) TSTAMP(6);
      f32x4 mv[NIT], rv[NIT];
      if constexpr (EPI == 3) {
        const auto mrs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.mask + img_off), 0, a.H * a.W * C * 4, 0x00020000);
        const auto rrs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.res + img_off), 0, a.H * a.W * C * 4, 0x00020000);
#pragma unroll
        for (int it = 0; it < NIT; ++it) {
          mv[it] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(mrs, yoff[it] + nr * 128, 0, 0));
          rv[it] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rrs, yoff[it] + nr * 128, 0, 0));
        }
      }
      const f32x4 i4 = inv_of(nr), b4 = bias_of(nr);
      f32x4 tv[NIT];
#pragma unroll
      for (int it = 0; it < NIT; ++it) tv[it] = xread(it);
      SB();
#pragma unroll
      for (int it = 0; it < NIT; ++it) {
        f32x4 v = tv[it] * i4 + b4;
        if (MASK) v = mask4(v, EPI == 3 ? mv[it] : op1[EPF ? nr : 0][it]);
        if (RES) v += EPI == 3 ? rv[it] : op1[EPF ? nr : 0][it];
        tv[it] = lrelu4(v, slope_eff);
      }
      SB();
      if (EPF && nr + 2 < NREP) load_op1(nr + 2);
      SB();                                          // (the operand requests stay above this slab's stores)
#if WX4_LEDGER & 512
#pragma unroll
      for (int it = 0; it < NIT; ++it) {                     // ledger probe NOSTORE: the epilogue without its global stores
#if defined(__HIP_DEVICE_COMPILE__)
        asm volatile("" ::"v"(tv[it]));
#endif
      }
      (void)yrs;
#else
      // (slab offset in the instruction's immediate, not in soffset: conv_f16.hip, store-data hazard of hipcc 7.2; the cache policy is an
      // immediate too: two copies of the eight stores behind a uniform branch)
      if (a.store_nt) {
#pragma unroll
        for (int it = 0; it < NIT; ++it) __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, tv[it]), yrs, yoff[it] + nr * 128, 0, 2);
      } else {
#pragma unroll
        for (int it = 0; it < NIT; ++it) __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, tv[it]), yrs, yoff[it] + nr * 128, 0, WX4_STORE_AUX);
      }
#endif
      if constexpr (TE) {
        const int cbg = (nbase >> 5) + nr;                  // 32-channel block of the stored tensor
        f32x4 cs = zero4;
        u32x4 uh[4], ul[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          float e8[8];
#pragma unroll
          for (int it = 0; it < NIT; ++it) {
            const float sv = yoff[it] != 0x80000000u ? tv[it][c] : 0.f;      // (tile pixels beyond the image are zero in T)
            cs[c] += sv;
            e8[it] = a.t_act ? fmaxf(sv, sv * a.t_slope) : sv;
          }
          t_units(e8, false, uh[c], ul[c]);
        }
        // Re-coalesce the slab's 4096 units through LDS (conv_f16_wx4h.hip): T's own order [row][plane][x-segment][32 ch], read back lane-linear
        wx_lds_barrier();
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          *reinterpret_cast<u32x4*>(xb + ((((te_row * 2 + 0) * 4 + te_xq) * 32 + 4 * cq + i) << 4)) = uh[i];
          *reinterpret_cast<u32x4*>(xb + ((((te_row * 2 + 1) * 4 + te_xq) * 32 + 4 * cq + i) << 4)) = ul[i];
        }
        wx_lds_barrier();
        {
          char* const tile0 = a.t_out + ((((size_t)img * (a.H + 2) + oy0 + 1) * a.t_cb + cbg) * a.t_npl * a.t_nseg + ((ox0 >> 3) + 1)) * 512;
          const size_t trow_bytes = (size_t)a.t_cb * a.t_npl * a.t_nseg * 512;
          const int uch = tid_e & 31, uxq = (tid_e >> 5) & 3, upl = (tid_e >> 7) & 1, urow = tid_e >> 8;   // unit u = k*512 + tid: row 2k + (tid>>8)
#pragma unroll
          for (int k = 0; k < 8; ++k) {
            const u32x4 v = *reinterpret_cast<const u32x4*>(xb + ((k * 512 + tid_e) << 4));
            const int r = 2 * k + urow;
            if (oy0 + r < a.H)
              *reinterpret_cast<u32x4*>(tile0 + r * trow_bytes + (size_t)upl * a.t_nseg * 512 + uxq * 512 + uch * 16) = v;
          }
        }
        if (a.t_col) {                                      // wave's channel sums (its 8 lanes per channel quad), one row per wave
#pragma unroll
          for (int c = 0; c < 4; ++c) {
            cs[c] += __shfl_xor(cs[c], 8);
            cs[c] += __shfl_xor(cs[c], 16);
            cs[c] += __shfl_xor(cs[c], 32);
          }
          if (lane_e < 8) *reinterpret_cast<f32x4*>(a.t_col + ((size_t)cbg * a.t_nblk + (size_t)tile * 8 + wave) * 32 + cq * 4) = cs;
        }
      }
      if (nr == 0) TSTAMP(7);
      if (nr + 1 < NREP) wx_lds_barrier();
    }
#ifdef WX4_PROBE_2X
    }
#endif
  } else {
    // generic form (two stored tensors and / or SFT on the output): optional operands by runtime pointer
    const char* const rimg = a.res ? reinterpret_cast<const char*>(a.res + img_off) : nullptr;
    const char* const mimg = a.mask ? reinterpret_cast<const char*>(a.mask + img_off) : nullptr;
    char* const yraw = a.y_raw ? reinterpret_cast<char*>(a.y_raw + img_off) : nullptr;
    char* const yact = a.y_act ? reinterpret_cast<char*>(a.y_act + img_off) : nullptr;
#pragma unroll
    for (int nr = 0; nr < NREP; ++nr) {
      xwrite(nr);
      wx_lds_barrier();
      const int co = nbase + nr * 32 + cq * 4;
      const f32x4 inv4 = inv_of(nr), bias4 = bias_of(nr);
      f32x4 mul4 = f32x4{1.f, 1.f, 1.f, 1.f}, add4 = zero4;
      if (a.mul) {                                           // SFT on the output (AttResUNet.py:57-58): SISR down path
        mul4 = *reinterpret_cast<const f32x4*>(a.mul + (size_t)img * C + co);
        add4 = *reinterpret_cast<const f32x4*>(a.add + (size_t)img * C + co);
      }
#pragma unroll
      for (int it = 0; it < NIT; ++it) {
        f32x4 v = xread(it) * inv4 + bias4;
        if (yoff[it] != 0x80000000u) {
          const unsigned o = yoff[it] + nr * 128;
          if (mimg) v = mask4(v, *reinterpret_cast<const f32x4*>(mimg + o));
          if (rimg) v += *reinterpret_cast<const f32x4*>(rimg + o);
          if (yraw) *reinterpret_cast<f32x4*>(yraw + o) = v;
          if (yact) *reinterpret_cast<f32x4*>(yact + o) = lrelu4(v * mul4 + add4, a.slope);
        }
      }
      if (nr + 1 < NREP) wx_lds_barrier();
    }
  }
  TSTAMP(3);
}

template <int NREP, int EPI, int PRE, int TE = 0>
int launch_wx4(FArgs k, hipStream_t st) {
  constexpr int LDS_K = WX_VBYTES + 2 * WX_UPIECES * NREP * 1024;
  constexpr int LDS_E = 24 * WX_XBLK;
  constexpr int LDS = (LDS_K > LDS_E ? LDS_K : LDS_E) + 2 * 32 * NREP * 4;      // + the channel block's inverse scales and biases
  static_assert(LDS <= 160 * 1024, "one workgroup per CU");
  static unsigned long long attr_done = 0;
  auto kern = conv_wx4_kernel<NREP, EPI, PRE, TE>;
  if (virnet::first_use_on_device(attr_done)) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    if (e != hipSuccess) return virnet::set_error("hipFuncSetAttribute(conv_wx4): %s", hipGetErrorString(e));
  }
  k.nty = (k.H + 15) / 16;
  k.ntx = (k.W + 31) / 32;
  k.ntiles = k.N * k.nty * k.ntx;
  k.tiles_per_xcd = (k.ntiles + 7) / 8;
  const int ncb = k.NP / (32 * NREP);
  const unsigned grid = (unsigned)(8 * k.tiles_per_xcd * ncb);
  if ((unsigned long long)grid * (unsigned)ncb >= (1ull << 32) || (unsigned long long)k.ntiles * (unsigned)(k.ntx * k.nty) >= (1ull << 32))
    return virnet::set_error("virnet_conv_wx4: %d tiles x %d channel blocks exceed the index arithmetic of one launch", k.ntiles, ncb);
  k.mg_ncb = div_magic(ncb);
  k.mg_ntx = div_magic(k.ntx);
  k.mg_tpi = div_magic(k.ntx * k.nty);
  hipLaunchKernelGGL(kern, dim3(grid), dim3(512), LDS + (PRE == 2 ? 2 * k.Cin * 4 : 0), st, k);      // (+ the image's SFT vectors)
  return virnet::check_launch("conv_wx4 launch");
}

#if !WX4_X1
// ---- weight packing ---------------------------------------------------------------------------------------------------------
// One block per GEMM row (output channel).  U[dy][j] = sum_b G[j][b] w[dy][b] in fp64, one power-of-two scale per row from the
// largest |U|, then the split image [slab][chunk][position j][dy][hi|lo][lane][8 x fp16] (lane / element order = the A fragment of
// v_mfma_f32_32x32x16_f16, as conv_f16.hip).  kind 0: forward OIHW; kind 2: the input-gradient GEMM (rows = forward cin, flipped taps).
__global__ void pack_wx4_kernel(const float* __restrict__ w, int kind, int cout, int cin, int cin_pad, int n_pad,
                                float* __restrict__ inv_scale, char* __restrict__ img) {
  const int row = blockIdx.x;
  const int rows = kind == 2 ? cin : cout, ks = kind == 2 ? cout : cin;
  const int nch = cin_pad >> 4;
  auto wval = [&](int k, int dy, int dx) -> double {
    if (row >= rows || k >= ks) return 0.0;
    return kind == 2 ? (double)w[(((size_t)k * cin + row) * 3 + (2 - dy)) * 3 + (2 - dx)] : (double)w[(((size_t)row * cin + k) * 3 + dy) * 3 + dx];
  };
  auto uval = [&](int k, int dy, int j) -> double {
    const double g0 = wval(k, dy, 0), g1 = wval(k, dy, 1), g2 = wval(k, dy, 2);
    switch (j) {
      case 0: return g0 * 0.25;
      case 1: return -(g0 + g1 + g2) / 6.0;
      case 2: return (-g0 + g1 - g2) / 6.0;
      case 3: return g0 / 24.0 + g1 / 12.0 + g2 / 6.0;
      case 4: return g0 / 24.0 - g1 / 12.0 + g2 / 6.0;
      default: return g2;
    }
  };
  __shared__ float red[256];
  float m = 0.f;
  for (int i = threadIdx.x; i < ks * 18; i += blockDim.x) m = fmaxf(m, fabsf((float)uval(i / 18, (i % 18) % 3, (i % 18) / 3)));
  red[threadIdx.x] = m;
  wx_lds_barrier();
  for (int s = 128; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) red[threadIdx.x] = fmaxf(red[threadIdx.x], red[threadIdx.x + s]);
    wx_lds_barrier();
  }
  m = red[0];
  int e = 0;
  if (m > 0.f) { frexpf(m, &e); e = 14 - e; }        // largest scaled magnitude in [8192, 16384)
  e = max(-100, min(100, e));
  if (threadIdx.x == 0) inv_scale[row] = ldexpf(1.f, -e);
  const int slab = row >> 5, col = row & 31;
  for (int i = threadIdx.x; i < cin_pad * 18; i += blockDim.x) {
    const int k = i / 18, t = i % 18, j = t / 3, dy = t % 3;
    const float v = (float)ldexp(uval(k, dy, j), e);
    const int chunk = k >> 4, kk = k & 15;
    const size_t base = (((((size_t)slab * nch + chunk) * 6 + j) * 3 + dy) * 2) * 1024 + (size_t)(col + 32 * (kk >> 3)) * 16 + (kk & 7) * 2;
    const _Float16 hi = (_Float16)v;
    *reinterpret_cast<_Float16*>(img + base) = hi;
    *reinterpret_cast<_Float16*>(img + base + 1024) = (_Float16)(v - (float)hi);
  }
}
#endif

}  // namespace

#if !WX4_X1

#ifdef VIRNET_F16_TIMING
extern long long* virnet_f16_tlog();
#endif

extern "C" size_t virnet_wx4_weight_floats(int cin_pad, int n_pad) { return (size_t)n_pad + (size_t)n_pad * cin_pad * 18; }

extern "C" int virnet_pack_wx4_weight(const float* w, int dgrad, int cout, int cin, int cin_pad, int n_pad, float* packed, void* stream) {
  VIRNET_REQUIRE(w && packed, "virnet_pack_wx4_weight: NULL pointer");
  VIRNET_REQUIRE(cout > 0 && cin > 0, "virnet_pack_wx4_weight: bad extents cout=%d cin=%d", cout, cin);
  const int rows = dgrad ? cin : cout, ks = dgrad ? cout : cin;
  VIRNET_REQUIRE(cin_pad % 16 == 0 && cin_pad >= ks, "virnet_pack_wx4_weight: cin_pad=%d does not cover %d contraction channels", cin_pad, ks);
  VIRNET_REQUIRE(n_pad % 32 == 0 && n_pad >= rows, "virnet_pack_wx4_weight: n_pad=%d does not cover %d output channels", n_pad, rows);
  hipLaunchKernelGGL(pack_wx4_kernel, dim3((unsigned)n_pad), dim3(256), 0, static_cast<hipStream_t>(stream), w, dgrad ? 2 : 0, cout, cin,
                     cin_pad, n_pad, packed, reinterpret_cast<char*>(packed + n_pad));
  return virnet::check_launch("pack_wx4 launch");
}

static int conv_wx4_impl(const virnet_conv_desc* d, void* stream, const virnet_t_emit* te);

// what the calling thread's most recent virnet_conv_wx4 / _emit call launched: {tile rows of its first launch (8 / 16), 1 if that launch was
// the persistent form, slabs per workgroup of the first launch, number of launches}
static thread_local int g_wx4_plan[4] = {0, 0, 0, 0};
extern "C" void virnet_conv_wx4_last_plan(int* out) {
  if (out) for (int i = 0; i < 4; ++i) out[i] = g_wx4_plan[i];
}

extern "C" int virnet_conv_wx4(const virnet_conv_desc* d, void* stream) { return conv_wx4_impl(d, stream, nullptr); }

int virnet::check_wx4_emit(const virnet_conv_desc* d, const virnet_t_emit* te) {
  VIRNET_REQUIRE(d != nullptr && te != nullptr && te->t_out != nullptr, "virnet_conv_wx4_emit: NULL descriptor / T buffer");
  int nblk = 0;
  VIRNET_REQUIRE(te->rows == 0 || te->rows == 8 || te->rows == 16, "virnet_conv_wx4_emit: rows=%d (0 / 16: 16-row tiles, 8: 8-row tiles)", te->rows);
  VIRNET_REQUIRE(virnet_conv_emit_ok(d, te->rows == 8 ? 2 : 1, &nblk), "virnet_conv_wx4_emit: T emission needs the stride-1 3x3 NHWC conv with ONE stored tensor, no output SFT and no in_mul");
  VIRNET_REQUIRE(!te->bf16, "virnet_conv_wx4_emit: the Winograd form has split-fp16 operands (T = fp16 hi | lo)");
  VIRNET_REQUIRE(!te->act || (te->slope >= 0.f && te->slope <= 1.f), "virnet_conv_wx4_emit: slope=%g outside [0,1]", te->slope);
  return 0;
}

extern "C" int virnet_conv_wx4_emit(const virnet_conv_desc* d, const virnet_t_emit* te, void* stream) {
  if (int rc = virnet::check_wx4_emit(d, te)) return rc;
  return conv_wx4_impl(d, stream, te);
}

// descriptor checks and the plan of its launches (conv_plan.h): the launch below and virnet_conv_plan_query.  n_cu <= 0: the device's
int virnet::plan_wx4_desc(const virnet_conv_desc* d, int emit_rows, int& n_cu, ConvKnobs& kn, ConvPlan& p) {
  VIRNET_REQUIRE(d != nullptr, "virnet_conv_wx4: desc is NULL");
  VIRNET_REQUIRE(d->x && d->wpack, "virnet_conv_wx4: x / wpack is NULL");
  VIRNET_REQUIRE(d->ks == 3 && d->stride == 1 && d->epi == VIRNET_EPI_NHWC, "virnet_conv_wx4: only the stride-1 3x3 NHWC conv (ks=%d stride=%d epi=%d)",
                 d->ks, d->stride, d->epi);
  if (int rc = check_conv_desc(d, "virnet_conv_wx4", true)) return rc;
  static int dev_cu = 0;
  if (n_cu <= 0) {
    if (dev_cu == 0) {
      int dev = 0;
      if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&dev_cu, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || dev_cu <= 0) dev_cu = 256;
    }
    n_cu = dev_cu;
  }
  const int nb = d->n_pad / 32;
  kn = read_conv_knobs(KNOBS_WX4, nb);
  FArgs k3{};                                            // the three-slab launch as the persistent form's admission sees it
  k3.Cin = d->cin_pad; k3.NP = slab_groups(nb).n3 * 96;
  const bool wx4p_ok = kn.wx4_persist && virnet::wx4p_serves(k3, 3, epi_of(d), pre_of(d));
  VIRNET_REQUIRE(plan_wx4(ConvShape{d->n, d->h, d->w, nb}, pre_of(d), emit_rows, kn, n_cu, wx4p_ok, p) == 0, "virnet_conv_wx4: more launches than a plan holds");
  return 0;
}

// one launch of the plan -> its template instantiation
static int launch_wx4_planned(const FArgs& kk, const ConvLaunch& l, int epi, int pre, bool te, int n_cu, hipStream_t st) {
  const int nrep = l.nrep;
#ifndef WX4_LEDGER_OFF_
  // ledger probe builds carry the two launch types of the metric's res-blocks only (conv1-type: PRE 1 / plain; conv2-type: residual)
  if (nrep == 3 && epi == 0 && pre == 1 && !te) return launch_wx4<3, 0, 1>(kk, st);
  if (nrep == 3 && epi == 1 && pre == 0 && !te) return launch_wx4<3, 1, 0>(kk, st);
  return virnet::set_error("virnet_conv_wx4: ledger probe build (WX4_LEDGER=%d) has no kernel for nrep=%d epi=%d pre=%d", WX4_LEDGER, nrep, epi, pre);
#else
  if (l.form == VIRNET_LAUNCH_WX4H) return te ? virnet::launch_wx4h_emit(kk, nrep, epi, pre, st) : virnet::launch_wx4h(kk, nrep, epi, pre, st);
  if (l.form == VIRNET_LAUNCH_WX4P) return virnet::launch_wx4p(kk, nrep, epi, pre, n_cu, st);
  if (te) {
#define VIRNET_WX4_TE(N_, E_) if (nrep == N_ && epi == E_) return pre == 1 ? launch_wx4<N_, E_, 1, 1>(kk, st) : launch_wx4<N_, E_, 0, 1>(kk, st);
#define VIRNET_WX4_TEN(N_) VIRNET_WX4_TE(N_, 0) VIRNET_WX4_TE(N_, 1) VIRNET_WX4_TE(N_, 2) VIRNET_WX4_TE(N_, 3)
    VIRNET_WX4_TEN(3) VIRNET_WX4_TEN(2) VIRNET_WX4_TEN(1)
#undef VIRNET_WX4_TEN
#undef VIRNET_WX4_TE
    return virnet::set_error("virnet_conv_wx4_emit: no emitting kernel for nrep=%d epi=%d pre=%d", nrep, epi, pre);
  }
#define VIRNET_WX4_EPI(N_, E_)                                                                                               \
  if (epi == E_) return pre == 2 ? launch_wx4<N_, E_, 2>(kk, st) : pre == 1 ? launch_wx4<N_, E_, 1>(kk, st) : launch_wx4<N_, E_, 0>(kk, st);
#define VIRNET_WX4_CASE(N_)                                                                              \
  if (nrep == N_) {                                                                                      \
    VIRNET_WX4_EPI(N_, 0) VIRNET_WX4_EPI(N_, 1) VIRNET_WX4_EPI(N_, 2) VIRNET_WX4_EPI(N_, 3) VIRNET_WX4_EPI(N_, 4)                          \
  }
  VIRNET_WX4_CASE(3) VIRNET_WX4_CASE(2) VIRNET_WX4_CASE(1)
#undef VIRNET_WX4_CASE
#undef VIRNET_WX4_EPI
  return virnet::set_error("virnet_conv_wx4: no kernel for nrep=%d", nrep);
#endif
}

static int conv_wx4_impl(const virnet_conv_desc* d, void* stream, const virnet_t_emit* te) {
  const bool te8 = te && te->rows == 8;                    // emitting form: 16-row tiles (8 waves) or 8-row tiles (4 waves, two workgroups per CU)
  ConvKnobs kn;
  ConvPlan p;
  int n_cu = 0;
  if (int rc = virnet::plan_wx4_desc(d, te ? (te8 ? 8 : 16) : 0, n_cu, kn, p)) return rc;
  FArgs k = fargs_from_desc(d);
#ifdef VIRNET_F16_TIMING
  k.tlog = virnet_f16_tlog();
#endif
  hipStream_t st = static_cast<hipStream_t>(stream);
  k.range_flag = virnet::range_flag_ptr();
  k.store_nt = virnet::store_nt_for((size_t)d->n * d->h * d->w * d->cout * 4);
  {
    // VIRNET_WX4_ALT=1 (probe): consecutive Winograd launches of a host thread walk their tiles in opposite directions, so that a conv starts
    // on the part of its input that its producer wrote last (still in the Infinity Cache)
    static thread_local int parity = 0;
    k.rev = kn.wx4_alt ? (parity ^= 1) : 0;
  }
#ifdef WX4_PROBE_2X
  k.nchw_op = getenv("WX4_PROBE_REPS") ? atoi(getenv("WX4_PROBE_REPS")) : 1;
#endif
  if (te) virnet::t_emit_args(k, te, d->w, d->cout, (int)(te8 ? tiles(d->n, d->h, d->w, 8) * 4 : tiles(d->n, d->h, d->w, 16) * 8));
  g_wx4_plan[0] = g_wx4_plan[1] = g_wx4_plan[2] = g_wx4_plan[3] = 0;
  const int epi = epi_of(d), pre = pre_of(d);
  for (int i = 0; i < p.n; ++i) {
#ifdef WX4_LEDGER_OFF_                                     // (launches attempted, as ever; a ledger probe build ignores the plan's forms and reports none)
    if (g_wx4_plan[3]++ == 0) { g_wx4_plan[0] = p.l[0].rows; g_wx4_plan[1] = p.l[0].persistent; g_wx4_plan[2] = p.l[0].nrep; }
#endif
    FArgs kk = k;
    kk.slab_base = p.l[i].slab_base;
    kk.NP = p.l[i].groups * p.l[i].nrep * 32;
    if (int rc = launch_wx4_planned(kk, p.l[i], epi, pre, te != nullptr, n_cu, st)) return rc;
  }
  return 0;
}
#endif  // !WX4_X1
