// DisentgBlock tail of DistgSSR at angRes 5 (model/SR/DistgSSR.py:84-99) in one launch: the second stages of the angular and both epipolar branches, the
// 144-channel concat and fuse.0 -- the concat never reaches HBM.
//   ang  = PS_5(lrelu(1x1 16 -> 400 (t_A)))                     channels  64 ..  79 of the concat
//   epiH = PS1D_5(lrelu(1x1 32 -> 160 (t_H)))                    channels  80 .. 111
//   epiV = PS1D_5(lrelu(1x1 32 -> 160 (t_V))), transposed        channels 112 .. 143
//   T    = lrelu(fuse.0 (spa | ang | epiH | epiV))               spa = channels 0 .. 63 = the SpaConv.2 output
// The stage-1 results t_A (B h w, 16), t_H (B A h w, 32, rows (b, u, y, x)) and t_V (rows (b, v, y, x)) come from the stage-1-only modes of k_ang_fused and
// k_epi_b3.  Work unit: a wave owns 16 macro-pixels (b, y, x) and walks their 25 views; everything a view's 16 output rows need is local to the tile:
// t_A of the 16 macro-pixels, t_H of row u, t_V of column v, and the 16 SpaConv.2 rows of the view.  Per view:
//   * AngConv.2: four v_mfma_f32_16x16x4_f32 exactly as k_ang_fused stage 2 (A = the t_A rows, B = the perm-1 W2 slice of the view);
//   * EPIConv.2 of both passes: 2 x 2 row tiles x six products of the three-term bf16 form exactly as k_epi_b3 stage 2 (A = the W2 planes of chunk v
//     (horizontal) / u (vertical), B = the t rows of the 16 macro-pixels in the lane order of k_epi_b3);
//   * the 80 branch channels of the 16 rows go through a wave-private LDS tile into B-operand order (lane = row, eight consecutive channels per k-group);
//   * fuse.0: 4 column tiles x 5 K steps x six products exactly as k_rowgemm_b3<160, false, 64, 144> (the SpaConv.2 rows loaded straight from HBM).
// Each accumulator sees the operands and the product order of the kernels it replaces (an MFMA's result column depends on its own B column only), so
// the output is bit-identical to the three-launch sequence.  The weights of all three GEMMs stay in LDS for the life of the block: fuse.0 60 KB (split
// once per block as k_rowgemm_b3 does), EPIConv.2 planes 30 KB (lfsr_pack_epi_b3), AngConv.2 25 KB; plus 8 x 5.25 KB of concat tiles.
#include "lfsr_internal.h"
#include <type_traits>

#ifndef DT_ABL
#define DT_ABL 0   // diagnostic timing build (WRONG results; tools/build_abl.sh, tools/tail_ab.py): 1 = every view's S / t_V / t_H loads go to the tile's view-0 rows (cache hits)
#endif

namespace {

typedef float f32x4t __attribute__((ext_vector_type(4)));
typedef unsigned u32x4t __attribute__((ext_vector_type(4)));

constexpr int DT_WAVES = 8;
constexpr int DT_FPLANE = 64 * 160;                  // bf16 per fuse.0 plane: [K step 5][k-group 4][row 64][8]
constexpr int DT_FBYTES = 3 * DT_FPLANE * 2;         // 61440
constexpr int DT_ESLOTS = 3 * 4 * 160;               // EPIConv.2 planes: [plane][k-group][n' 160] 16-B slots (as k_epi_b3)
constexpr int DT_EBYTES = DT_ESLOTS * 16;            // 30720
constexpr int DT_AFLOATS = 25 * 16 * 16;             // AngConv.2, perm 1: [view * 16 + c][16]
constexpr int DT_ABYTES = DT_AFLOATS * 4;            // 25600
constexpr int DT_CROW = 84;                          // concat tile row: ang 0..15 | epiH 16..47 | epiV 48..79 (+ 4 pad)
constexpr int DT_CBYTES = DT_WAVES * 16 * DT_CROW * 4;   // 43008
constexpr int DT_SMEM = DT_FBYTES + DT_EBYTES + DT_ABYTES + DT_CBYTES;   // 160768

struct DistgTailArgs {
  const float* S; int s_stride; int s_choff; int s_bytes;     // SpaConv.2 output, VCL
  const float* TA; int ta_bytes;                              // (B h w, 16)
  const float* TH; const float* TV; int te_bytes;             // (B A h w, 32) each
  const float* WA2;                                           // AngConv.2, perm-1 pack
  const uint4* WE2p;                                          // EPIConv.2 planes (lfsr_pack_epi_b3 kind 1)
  const float* WF;                                            // fuse.0, packed [64][144]
  float* Y; int y_stride; int y_choff; int y_bytes;           // T, VCL
  int B, H, W;
  float slope;
};

__device__ __forceinline__ void dt_split8(const f32x4t lo, const f32x4t hi, u32x4t& p0, u32x4t& p1, u32x4t& p2) {
  const float a[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
#pragma unroll
  for (int j = 0; j < 4; ++j) { unsigned t0, t1, t2; lfsr_split_pair(a[2 * j], a[2 * j + 1], t0, t1, t2); p0[j] = t0; p1[j] = t1; p2[j] = t2; }
}

// asm MFMA with the accumulator tied (rowgemm_b3.hip, b3_mfma: why not the builtin)
__device__ __forceinline__ void dt_mfma(f32x4t& c, const u32x4t a, const u32x4t b) {
  asm volatile("v_mfma_f32_16x16x32_bf16 %0, %1, %2, %0" : "+v"(c) : "v"(a), "v"(b));
}

// the six products of one accumulator in the order of k_epi_b3 / k_rowgemm_b3 (smallest terms first); two accumulators interleaved
__device__ __forceinline__ void dt_six2(f32x4t& c0, const u32x4t (&a)[3], const u32x4t (&x)[3], f32x4t& c1, const u32x4t (&b)[3], const u32x4t (&y)[3]) {
  dt_mfma(c0, a[2], x[0]); dt_mfma(c1, b[2], y[0]);
  dt_mfma(c0, a[0], x[2]); dt_mfma(c1, b[0], y[2]);
  dt_mfma(c0, a[1], x[1]); dt_mfma(c1, b[1], y[1]);
  dt_mfma(c0, a[1], x[0]); dt_mfma(c1, b[1], y[0]);
  dt_mfma(c0, a[0], x[1]); dt_mfma(c1, b[0], y[1]);
  dt_mfma(c0, a[0], x[0]); dt_mfma(c1, b[0], y[0]);
}

__global__ __launch_bounds__(512) void k_distg_tail(DistgTailArgs p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  unsigned short* const sF = reinterpret_cast<unsigned short*>(smem_raw);
  unsigned char* const sE = smem_raw + DT_FBYTES;
  float* const sA = reinterpret_cast<float*>(smem_raw + DT_FBYTES + DT_EBYTES);
  float* const sC = reinterpret_cast<float*>(smem_raw + DT_FBYTES + DT_EBYTES + DT_ABYTES);
  constexpr int A = 5, AA = 25;
  constexpr int EOOB = (int)0x80000000u;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l15 = lane & 15, g = lane >> 4;
  const int HW = p.H * p.W, M = p.B * HW;
  const int ntiles = (M + 15) / 16;

  const __amdgpu_buffer_rsrc_t rsS = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.S), 0, p.s_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t rsA = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.TA), 0, p.ta_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t rsH = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.TH), 0, p.te_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t rsV = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.TV), 0, p.te_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t rsY = __builtin_amdgcn_make_buffer_rsrc(p.Y, 0, p.y_bytes, 0x00020000);

  // A tile's place in the three operands.  lane (l15, g): macro-pixel m = 16 tile + l15 -- the B-operand column of the bf16 MFMAs (and the A row of the fp32
  // ones).  A tile past the end (a wave without work, the hand-over behind a wave's last tile) has no row in range: every load of it moves no data.
  struct Tile { bool ok; int ao, tb, pb; };      // t_A byte offset; t_H / t_V row of (b, 0, y, x); VCL pixel of view 0
  auto place = [&](int tile) {
    const int m = tile * 16 + l15;
    Tile c;
    c.ok = tile < ntiles && m < M;
    const int mb = c.ok ? m / HW : 0, myx = c.ok ? m - mb * HW : 0;
    c.ao = c.ok ? (m * 16 + 4 * g) * 4 : EOOB;
    c.tb = mb * A * HW + myx;
    c.pb = mb * AA * HW + myx;
    return c;
  };
  auto tro = [&](const Tile& c, int q) {        // t_H / t_V row (b, q, y, x): channels 4 g .. + 3 (+ 64 B: 16 + 4 g)
    if (DT_ABL & 1) q = 0;
    return c.ok ? ((c.tb + q * HW) * 32 + 4 * g) * 4 : EOOB;
  };
  auto pixo = [&](const Tile& c, int view) { return c.ok ? c.pb + view * HW : -1; };            // VCL pixel of this lane's row in a view

  // raw operands of one view: the SpaConv.2 row (K steps 0, 1: lo / hi four floats) and the t_V row, double-buffered: a body requests the next view's rows
  // first and waits only for its own (requested one body earlier), so six to eight loads and the previous body's four stores stay outstanding under its
  // MFMAs.  No load sits behind a run-time branch: a row that is not wanted gets an out-of-range offset (no data moves), so the compiler counts every wait.
  f32x4t sr0[2][2], sr1[2][2], vr0[2], vr1[2], hr[2], a2n;
  auto load_view = [&](const Tile& c, int view, f32x4t (&sr)[2][2], f32x4t (&vr)[2]) {
    const int pix = pixo(c, (DT_ABL & 1) ? 0 : view);
    const int so = pix >= 0 ? (pix * p.s_stride + p.s_choff + 8 * g) * 4 : EOOB;
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
      for (int e = 0; e < 2; ++e) sr[s][e] = __builtin_bit_cast(f32x4t, __builtin_amdgcn_raw_buffer_load_b128(rsS, so == EOOB ? EOOB : so + (32 * s + 4 * e) * 4, 0, 0));
    const int vo = tro(c, view % A);
    vr[0] = __builtin_bit_cast(f32x4t, __builtin_amdgcn_raw_buffer_load_b128(rsV, vo, 0, 0));
    vr[1] = __builtin_bit_cast(f32x4t, __builtin_amdgcn_raw_buffer_load_b128(rsV, vo == EOOB ? EOOB : vo + 64, 0, 0));
  };
  auto load_h = [&](int ho) {
    hr[0] = __builtin_bit_cast(f32x4t, __builtin_amdgcn_raw_buffer_load_b128(rsH, ho, 0, 0));
    hr[1] = __builtin_bit_cast(f32x4t, __builtin_amdgcn_raw_buffer_load_b128(rsH, ho == EOOB ? EOOB : ho + 64, 0, 0));
  };
  auto load_first = [&](const Tile& c) {        // what a tile needs before its first view: t_A, view 0, t_H row 0
    a2n = __builtin_bit_cast(f32x4t, __builtin_amdgcn_raw_buffer_load_b128(rsA, c.ao, 0, 0));   // t_A row m, k = 4 g .. + 3
    load_view(c, 0, sr0, vr0);
    load_h(tro(c, 0));
  };

  // the wave's first tile is requested before the weights: the staging and its barrier no longer sit in front of every byte the wave streams
  int tile = (int)blockIdx.x * DT_WAVES + wave;
  Tile nx = place(tile);
  load_first(nx);

  // ---- weights, once per block ----
  for (int i = tid; i < 64 * 20; i += 512) {       // fuse.0: split into planes as k_rowgemm_b3 (KV = 144 of K = 160; columns >= 144 zero)
    const int r = i / 20, c = i - r * 20;
    const bool ok = c * 8 < 144;
    const float* src = p.WF + r * 144 + (ok ? c * 8 : 0);
    f32x4t lo = *reinterpret_cast<const f32x4t*>(src), hi = *reinterpret_cast<const f32x4t*>(src + 4);
    if (!ok) { lo = f32x4t{0.f, 0.f, 0.f, 0.f}; hi = lo; }
    u32x4t w0, w1, w2;
    dt_split8(lo, hi, w0, w1, w2);
    const int slot = (c * 64 + r) * 8;
    *reinterpret_cast<u32x4t*>(sF + 0 * DT_FPLANE + slot) = w0;
    *reinterpret_cast<u32x4t*>(sF + 1 * DT_FPLANE + slot) = w1;
    *reinterpret_cast<u32x4t*>(sF + 2 * DT_FPLANE + slot) = w2;
  }
  for (int i = tid; i < DT_ESLOTS; i += 512) reinterpret_cast<uint4*>(sE)[i] = p.WE2p[i];
  for (int i = tid; i < DT_AFLOATS / 4; i += 512) reinterpret_cast<float4*>(sA)[i] = reinterpret_cast<const float4*>(p.WA2)[i];
  __syncthreads();

  float* const st = sC + wave * 16 * DT_CROW;                          // this wave's concat tile [row][DT_CROW]
  const unsigned char* const wE = sE + (g * 160 + l15) * 16;           // EPIConv.2 A operand: k-group g, row l15 (+ 16 per row tile, + 640 slots per plane)
  const unsigned short* const wF = sF + (g * 64 + l15) * 8;            // fuse.0 A operand: k-group g, row l15 (+ 16 rows per column tile, + 256 slots per K step)
  const float* const bA = sA + l15 * 16 + 4 * g;                       // AngConv.2 B operand (+ 256 per view)

  for (; tile < ntiles; tile += (int)gridDim.x * DT_WAVES) {
    const Tile cur = nx;
    const f32x4t a2 = a2n;
    u32x4t hp[3];                        // planes of t_H (row u of the current view)

    // LAST is a property of the body's copy, not of the view: the two bodies of the loop always have a next view in their own tile, the trailing one requests
    // the first rows of the wave's next tile (out of range when there is none) once its own are split.
    auto body = [&](int view, f32x4t (&sr)[2][2], f32x4t (&vr)[2], f32x4t (&srn)[2][2], f32x4t (&vrn)[2], auto last) {
      constexpr bool LAST = decltype(last)::value;
      const int u = view / A, v = view - A * u;
      // LDS operands are read one MFMA group ahead of their use (an LDS read stays where the source puts it between the asm MFMAs): read in front of its own
      // group, every one of the 13 groups of a view began with an LDS round trip that nothing covered
      const float4 b = *reinterpret_cast<const float4*>(bA + view * 256);      // AngConv.2 B operand
      if constexpr (LAST) a2n = __builtin_bit_cast(f32x4t, __builtin_amdgcn_raw_buffer_load_b128(rsA, nx.ao, 0, 0));
      else load_view(cur, view + 1, srn, vrn);
      if (v == 0) dt_split8(hr[0], hr[1], hp[0], hp[1], hp[2]);        // (before the t_H request below: that one lands in hr)
      load_h(LAST ? tro(nx, 0) : v == A - 1 && u + 1 < A ? tro(cur, u + 1) : EOOB);      // row u + 1 during the last view of row u; nothing otherwise
      // ---- AngConv.2 of this view (k_ang_fused stage 2): D[macro-pixel 4 g + r][channel l15] ----
      {
        f32x4t o = {0.f, 0.f, 0.f, 0.f};
        o = __builtin_amdgcn_mfma_f32_16x16x4f32(a2.x, b.x, o, 0, 0, 0);
        o = __builtin_amdgcn_mfma_f32_16x16x4f32(a2.y, b.y, o, 0, 0, 0);
        o = __builtin_amdgcn_mfma_f32_16x16x4f32(a2.z, b.z, o, 0, 0, 0);
        o = __builtin_amdgcn_mfma_f32_16x16x4f32(a2.w, b.w, o, 0, 0, 0);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          float z = o[r];
          z = z >= 0.f ? z : z * p.slope;
          st[(4 * g + r) * DT_CROW + l15] = z;
        }
      }

      // ---- EPIConv.2 of both passes (k_epi_b3 stage 2): horizontal = chunk v of t_H (row u), vertical = chunk u of t_V (column v) ----
      {
        u32x4t aH[2][3], aV[2][3];
        auto load_we = [&](int h) {
#pragma unroll
          for (int pl = 0; pl < 3; ++pl) {
            aH[h][pl] = *reinterpret_cast<const u32x4t*>(wE + ((pl * 4) * 160 + 16 * (2 * v + h)) * 16);
            aV[h][pl] = *reinterpret_cast<const u32x4t*>(wE + ((pl * 4) * 160 + 16 * (2 * u + h)) * 16);
          }
        };
        load_we(0);
        u32x4t vp[3];
        dt_split8(vr[0], vr[1], vp[0], vp[1], vp[2]);
        asm volatile("s_nop 4" : "+v"(hp[0]), "+v"(hp[1]), "+v"(hp[2]), "+v"(vp[0]), "+v"(vp[1]), "+v"(vp[2]));
        f32x4t e[2][2];                  // [pass][row tile h]: channels 16 h + 4 g + r of macro-pixel l15
#pragma unroll
        for (int i = 0; i < 2; ++i) { e[i][0] = f32x4t{0.f, 0.f, 0.f, 0.f}; e[i][1] = e[i][0]; }
        asm volatile("s_nop 1" : "+v"(e[0][0]), "+v"(e[0][1]), "+v"(e[1][0]), "+v"(e[1][1]));
        load_we(1);
        dt_six2(e[0][0], aH[0], hp, e[1][0], aV[0], vp);
        dt_six2(e[0][1], aH[1], hp, e[1][1], aV[1], vp);
        asm volatile("s_nop 15\n\ts_nop 15" : "+v"(e[0][0]), "+v"(e[0][1]), "+v"(e[1][0]), "+v"(e[1][1]));
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
          for (int h = 0; h < 2; ++h) {
            f32x4t z = e[i][h];
#pragma unroll
            for (int r = 0; r < 4; ++r) z[r] = fmaxf(z[r], z[r] * p.slope);
            *reinterpret_cast<f32x4t*>(st + l15 * DT_CROW + 16 + 32 * i + 16 * h + 4 * g) = z;
          }
      }
      __builtin_amdgcn_wave_barrier();

      // ---- fuse.0 (k_rowgemm_b3<160, false, 64, 144>): B operand = row l15, channels 32 s + 8 g .. + 7 ----
      u32x4t wa[2][3], wb[2][3];         // fuse.0 A operands of group gi = 2 s + t / 2 (K step s, column tiles t, t + 1), double-buffered
      auto load_wf = [&](int gi) {
        const int s = gi >> 1, t = 2 * (gi & 1);
#pragma unroll
        for (int pl = 0; pl < 3; ++pl) {
          wa[gi & 1][pl] = *reinterpret_cast<const u32x4t*>(wF + pl * DT_FPLANE + (4 * s * 64 + t * 16) * 8);
          wb[gi & 1][pl] = *reinterpret_cast<const u32x4t*>(wF + pl * DT_FPLANE + (4 * s * 64 + (t + 1) * 16) * 8);
        }
      };
      load_wf(0);
      u32x4t x0[5], x1[5], x2[5];
#pragma unroll
      for (int s = 0; s < 2; ++s) dt_split8(sr[s][0], sr[s][1], x0[s], x1[s], x2[s]);
#pragma unroll
      for (int s = 2; s < 5; ++s) {
        const float* cp = st + l15 * DT_CROW + 32 * (s - 2) + 8 * g;
        f32x4t lo = *reinterpret_cast<const f32x4t*>(cp), hi = *reinterpret_cast<const f32x4t*>(cp + 4);
        if (s == 4 && g >= 2) { lo = f32x4t{0.f, 0.f, 0.f, 0.f}; hi = lo; }      // channels 144 .. 159: zero operand columns
        dt_split8(lo, hi, x0[s], x1[s], x2[s]);
      }
      __builtin_amdgcn_wave_barrier();
      f32x4t acc[4];
#pragma unroll
      for (int t = 0; t < 4; ++t) acc[t] = f32x4t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int s = 0; s < 5; ++s) asm volatile("s_nop 4" : "+v"(x0[s]), "+v"(x1[s]), "+v"(x2[s]));
      asm volatile("s_nop 1" : "+v"(acc[0]), "+v"(acc[1]), "+v"(acc[2]), "+v"(acc[3]));
      if constexpr (LAST) load_view(nx, 0, sr, vr);      // 25 views: the next tile starts in the set this view has just split, so its rows fly under fuse.0
#pragma unroll
      for (int gi = 0; gi < 10; ++gi) {
        const int s = gi >> 1, t = 2 * (gi & 1);
        const u32x4t xs[3] = {x0[s], x1[s], x2[s]};
        if (gi + 1 < 10) load_wf(gi + 1);
        dt_six2(acc[t], wa[gi & 1], xs, acc[t + 1], wb[gi & 1], xs);
      }
      asm volatile("s_nop 15\n\ts_nop 15" : "+v"(acc[0]), "+v"(acc[1]), "+v"(acc[2]), "+v"(acc[3]));
      const int pix = pixo(cur, view);
      const int yo = pix >= 0 ? (pix * p.y_stride + p.y_choff + 4 * g) * 4 : EOOB;
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        f32x4t z = acc[t];
#pragma unroll
        for (int r = 0; r < 4; ++r) z[r] = z[r] >= 0.f ? z[r] : z[r] * p.slope;
        __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4t, z), rsY, yo == EOOB ? EOOB : yo + 64 * t, 0, 0);
        asm volatile("s_nop 1" : "+v"(z));      // (store data -> a later asm MFMA writing the same registers: k_epi_b3's store hazard)
      }
    };
#pragma unroll 1
    for (int view = 0; view < AA - 1; view += 2) {
      body(view, sr0, vr0, sr1, vr1, std::false_type{});
      body(view + 1, sr1, vr1, sr0, vr0, std::false_type{});
    }
    nx = place(tile + (int)gridDim.x * DT_WAVES);
    body(AA - 1, sr0, vr0, sr1, vr1, std::true_type{});
  }
}

}  // namespace

// t_a / t_h / t_v: the stage-1 results (k_ang_fused / k_epi_b3 stage-1-only modes); spa: the SpaConv.2 output; y: fuse.0's output.  LFSR_E_ARG = not covered.
int lfsr_distg_tail_launch(const LfsrDistgTail& t, hipStream_t st) {
  const int B = t.B, A = t.A, h = t.h, w = t.w;
  const float* we2_planes = t.w_epi2_planes();
  if (A != 5 || B <= 0 || h <= 0 || w <= 0 || !t.spa || !t.t_a || !t.t_h || !t.t_v || !t.w_ang2 || !we2_planes || !t.w_fuse0 || !t.y) return LFSR_E_ARG;
  if ((t.spa_stride | t.spa_choff | t.y_stride | t.y_choff) & 3 || t.spa_stride < t.spa_choff + 64 || t.y_stride < t.y_choff + 64) return LFSR_E_ARG;
  if (((uintptr_t)t.spa | (uintptr_t)t.t_a | (uintptr_t)t.t_h | (uintptr_t)t.t_v | (uintptr_t)t.w_ang2 | (uintptr_t)we2_planes | (uintptr_t)t.w_fuse0 | (uintptr_t)t.y) & 15)
    return LFSR_E_ARG;
  if (!(t.slope >= 0.f && t.slope <= 1.f)) return LFSR_E_ARG;      // LeakyReLU as max(v, slope v) in the epipolar stage (as k_epi_b3)
  const long long npix = (long long)B * A * A * h * w;
  if (npix * t.spa_stride * 4 >= (1LL << 31) || npix * t.y_stride * 4 >= (1LL << 31) || (long long)B * A * h * w * 32 * 4 >= (1LL << 31)) return LFSR_E_ARG;   // 32-bit byte offsets
  static std::atomic<bool> attr_set[64];
  static std::atomic<int> cus[64];
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return LFSR_HIP_ERR(hipErrorInvalidDevice);
  if (!attr_set[dev]) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(k_distg_tail), hipFuncAttributeMaxDynamicSharedMemorySize, DT_SMEM);
    if (e != hipSuccess) return LFSR_HIP_ERR(e);
    int v = 0;
    cus[dev] = (hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && v > 0) ? v : 256;
    attr_set[dev] = true;
  }
  DistgTailArgs p{};
  p.S = t.spa; p.s_stride = t.spa_stride; p.s_choff = t.spa_choff; p.s_bytes = (int)(npix * t.spa_stride * 4);
  p.TA = t.t_a; p.ta_bytes = (int)((long long)B * h * w * 16 * 4);
  p.TH = t.t_h; p.TV = t.t_v; p.te_bytes = (int)((long long)B * A * h * w * 32 * 4);
  p.WA2 = t.w_ang2; p.WE2p = reinterpret_cast<const uint4*>(we2_planes); p.WF = t.w_fuse0;
  p.Y = t.y; p.y_stride = t.y_stride; p.y_choff = t.y_choff; p.y_bytes = (int)(npix * t.y_stride * 4);
  p.B = B; p.H = h; p.W = w; p.slope = t.slope;
  const long long ntiles = ((long long)B * h * w + 15) / 16;
  long long grid = (ntiles + DT_WAVES - 1) / DT_WAVES;
  if (grid > cus[dev]) grid = cus[dev];
  hipLaunchKernelGGL(k_distg_tail, dim3((unsigned)grid), dim3(DT_WAVES * 64), DT_SMEM, st, p);
  LFSR_CHECK_LAUNCH();
  return LFSR_OK;
}
