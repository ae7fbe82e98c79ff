// DistgSSR's EPI branch (stage 1) and DisentgBlock tail at angRes 5 on bf16 OPERANDS: lfsr_set_branch_arithmetic(LFSR_BRANCH_ARITH_BF16), opt-in.  The
// counterparts of k_epi_b3<false> (epi_b3.hip) and k_distg_tail (distg_tail.hip), which carry every fp32 operand exactly as three bf16 terms: six MFMA products
// per K step plus the VALU work of the split.  Here an operand is rounded to bf16 ONCE (v_cvt_pk_bf16_f32: nearest even) and every K step is one product:
//   * EPIConv.0, both passes: x and the weight;
//   * EPIConv.2, both passes: t_H / t_V (the fp32 post-LeakyReLU stage-1 results as they lie in memory) and the weight;
//   * fuse.0: all 144 concat channels (the SpaConv.2 rows, the post-LeakyReLU AngConv.2 and EPIConv.2 results) and the weight.
// Products are exact (v_mfma_f32_16x16x32_bf16); accumulation, LeakyReLU and stores are fp32; t_A, t_H, t_V and y stay fp32 in memory.  AngConv.2 keeps its
// fp32-MFMA arithmetic.  The weights are rounded while a block stages them into LDS, once per block, from the fp32 packs (never from plane 0 of the three-term
// packs, which is a truncation): no new pack, no new workspace.
//
// k_epi_bf16: the formulation of k_epi_b3 (N = source positions, five shifted accumulator tiles summed by DPP row shifts, one wave per EPI line, x loaded straight
// from global memory in B-operand order).  With one plane the whole EPIConv.0 weight is 25 x 32 x 64 x 2 B = 100 KB and stays in LDS for the life of the block as
// [step 2 v' + ks][dx][k-group][row] 16-B slots (eight consecutive k per slot: the conflict-free image of gemm_bf16.hip), so the per-view staging and its barrier
// are gone: the only barrier is the one behind the staging.  20 MFMAs per step instead of 120.
// k_distg_tail_bf16: the work unit of k_distg_tail (a wave owns 16 macro-pixels and walks their 25 views, operands double-buffered one view ahead, no load behind
// a run-time branch).  Per view 4 fp32 MFMAs (AngConv.2) + 4 (EPIConv.2) + 20 (fuse.0) bf16 products instead of 144.  The 80 branch channels of the 16 rows go
// through a wave-private LDS tile ALREADY ROUNDED (bf16: their one rounding), so fuse.0 reads them back as B operands with no conversion.  LDS: fuse.0 20 KB +
// EPIConv.2 10 KB + AngConv.2 25 KB (fp32) + 8 x 2.75 KB of concat tiles = 77 KB: two blocks per CU (launch bounds (512, 2): at most 128 VGPRs), i.e. four
// waves per SIMD instead of two to cover a kernel that is now bound by its loads.
// No atomics in either kernel: two runs give the same bits, and a line's / macro-pixel's result depends on neither B nor the grid.
#include "lfsr_internal.h"
#include <type_traits>

namespace {

typedef float f32x4b __attribute__((ext_vector_type(4)));
typedef unsigned u32x4b __attribute__((ext_vector_type(4)));
typedef unsigned u32x2b __attribute__((ext_vector_type(2)));

__device__ __forceinline__ unsigned bb_cvt_pk(float lo, float hi) {
  unsigned r;
  asm("v_cvt_pk_bf16_f32 %0, %1, %2" : "=v"(r) : "v"(lo), "v"(hi));
  return r;
}
// eight consecutive floats -> one bf16 MFMA operand (element 0 in the low half)
__device__ __forceinline__ u32x4b bb_cvt8(const f32x4b lo, const f32x4b hi) {
  return u32x4b{bb_cvt_pk(lo.x, lo.y), bb_cvt_pk(lo.z, lo.w), bb_cvt_pk(hi.x, hi.y), bb_cvt_pk(hi.z, hi.w)};
}
// asm MFMA with the accumulator tied (rowgemm_b3.hip, b3_mfma: why not the builtin)
__device__ __forceinline__ void bb_mfma(f32x4b& c, const u32x4b a, const u32x4b b) {
  asm volatile("v_mfma_f32_16x16x32_bf16 %0, %1, %2, %0" : "+v"(c) : "v"(a), "v"(b));
}

// =====================================================================================================================================================
// EPI stage 1
// =====================================================================================================================================================
constexpr int EK_LINES = 8;
constexpr int EK_STEP_SLOTS = 5 * 4 * 32;                    // 16-B slots of one step (view v', K step ks): [dx][k-group][n]
constexpr int EK_STEP_BYTES = EK_STEP_SLOTS * 16;            // 10240
constexpr int EK_SLOTS = 10 * EK_STEP_SLOTS;                 // 6400
constexpr int EK_SMEM = EK_SLOTS * 16;                       // 102400

struct EpiBf16Args {
  const float* X; int x_stride; int x_choff; int x_bytes;
  const float* W1;        // EPIConv.0 direct pack, fp32: [tap 5 dx + v'][n 32][c 64]
  float* TH; float* TV; int te_bytes;   // (lines * len, 32) each
  int B, H, W;
  int tilesH, tilesV;     // groups per pass
  int tpiH, tpiV;         // > 0: groups ordered item by item (an item's horizontal groups, then its vertical ones)
  float slope;
};

// lane i of a row of 16 reads lane i + N (row_shl) / i - N (row_shr) of the same row; lanes that would read outside the row get 0
template <int CTRL>
__device__ __forceinline__ float ek_dpp0(float v) {
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xf, 0xf, true));
}
// z[x + D] for the two position tiles of a line (epi_b3.hip, eb_shift_add)
template <int D>
__device__ __forceinline__ void ek_shift_add(f32x4b (&t)[2], const f32x4b (&z)[2]) {
  constexpr int SAME = D > 0 ? 0x100 + D : 0x110 - D;                 // row_shl:D / row_shr:-D
  constexpr int WRAP = D > 0 ? 0x110 + (16 - D) : 0x100 + (16 + D);   // row_shr:(16 - D) / row_shl:(16 + D)
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    t[0][r] += ek_dpp0<SAME>(z[0][r]);
    t[1][r] += ek_dpp0<SAME>(z[1][r]);
    if (D > 0) t[0][r] += ek_dpp0<WRAP>(z[1][r]);
    else t[1][r] += ek_dpp0<WRAP>(z[0][r]);
  }
}

__global__ __launch_bounds__(512) void k_epi_bf16(EpiBf16Args p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  unsigned char* const sW = smem_raw;                                   // [step 10][EK_STEP_BYTES]
  constexpr int A = 5;
  constexpr int EOOB = (int)0x80000000u;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l15 = lane & 15, g = lane >> 4;
  const int phase = __builtin_amdgcn_readfirstlane(wave >> 2);     // the two waves of a SIMD: 0 / 1
  const int HW = p.H * p.W;
  const int ngroups = p.tilesH + p.tilesV;
  // consecutive workgroups go to consecutive XCDs: the blocks of one XCD walk a contiguous range of groups (both passes of an item share an L2)
  const int nb = (int)gridDim.x;
  const int vb = (nb & 7) ? (int)blockIdx.x : ((int)blockIdx.x & 7) * (nb >> 3) + ((int)blockIdx.x >> 3);

  const __amdgpu_buffer_rsrc_t rsX = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.X), 0, p.x_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t rsH = __builtin_amdgcn_make_buffer_rsrc(p.TH, 0, p.te_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t rsV = __builtin_amdgcn_make_buffer_rsrc(p.TV, 0, p.te_bytes, 0x00020000);

  // ---- group geometry (block-uniform) and this wave's line: the work units of k_epi_b3 (whole groups of 8 lines; the groups left over after the last full
  //      round cut into 2 or 4 sub-groups while they still fit one round) ----
  struct Line { int vert, base, len, vstride, pstride, row, rowstep; };
  const int nfr = ngroups / nb, nfull = nfr * nb, rem = ngroups - nfull;
  const int fsub = rem == 0 ? 1 : (rem * 4 <= nb ? 4 : rem * 2 <= nb ? 2 : 1);
  const int nunits = nfr + (vb < rem * fsub ? 1 : 0);                 // (block-uniform)
  auto line_of = [&](int it) -> Line {
    Line L;
    int grp, l0 = 0, nl = EK_LINES;
    if (it < nfr) grp = vb + it * nb;
    else if (it < nunits) { grp = nfull + vb / fsub; nl = EK_LINES / fsub; l0 = (vb % fsub) * nl; }
    else grp = ngroups;                                                 // past the end: an absent line, every access out of range
    int tile;
    if (p.tpiH > 0) {
      const int per = p.tpiH + p.tpiV, item = grp / per, r = grp - item * per;
      L.vert = r >= p.tpiH;
      tile = L.vert ? item * p.tpiV + (r - p.tpiH) : item * p.tpiH + r;
    } else {
      L.vert = grp >= p.tilesH;
      tile = L.vert ? grp - p.tilesH : grp;
    }
    L.len = L.vert ? p.H : p.W;
    const int across = L.vert ? p.W : p.H;
    const int nlines = p.B * A * across;
    L.vstride = L.vert ? A * HW : HW;
    L.pstride = L.vert ? p.W : 1;
    const int ln = tile * EK_LINES + l0 + wave;
    L.base = -1; L.row = 0; L.rowstep = 0;
    if (grp < ngroups && wave < nl && ln < nlines) {
      const int q = ln / across, o = ln - q * across;     // horizontal: q = b*A+u, o = y;  vertical: q = b*A+v, o = x
      if (!L.vert) L.base = q * A * HW + o * p.W;
      else { const int b = q / A, v = q - b * A; L.base = (b * A * A + v) * HW + o; }
      // rows of the stage-1 matrix: (b*A+u, y, x) / (b*A+v, y, x)
      L.row = L.vert ? q * HW + o : (q * p.H + o) * p.W;
      L.rowstep = L.vert ? p.W : 1;
    }
    return L;
  };

  // raw input two steps deep ([source tile nt][lo / hi four floats]) and its bf16 operands, double-buffered: step j's MFMAs read one set while the raw values of
  // step j + 1 are converted into the other and the loads of step j + 2 fly
  f32x4b rawA[2][2], rawB[2][2];
  u32x4b pA[2], pB[2];
  auto load_x = [&](int base, int len, int vstride, int pstride, int j, f32x4b (&xr)[2][2]) {   // step j = 2 v' + ks of the line
    const int vv = j >> 1, ks = j & 1;
    const int soff = (vv * vstride * p.x_stride + 32 * ks) * 4;
#pragma unroll
    for (int nt = 0; nt < 2; ++nt) {
      const int s = 16 * nt + l15;
      const int off = (base >= 0 && s < len) ? ((base + s * pstride) * p.x_stride + p.x_choff + 8 * g) * 4 : EOOB;
      xr[nt][0] = __builtin_bit_cast(f32x4b, __builtin_amdgcn_raw_buffer_load_b128(rsX, off, soff, 0));
      xr[nt][1] = __builtin_bit_cast(f32x4b, __builtin_amdgcn_raw_buffer_load_b128(rsX, off == EOOB ? EOOB : off + 16, soff, 0));
    }
  };

  if (nunits == 0) return;              // (block-uniform: before the barrier)
  int it = 0;
  Line L = line_of(0);
  load_x(L.base, L.len, L.vstride, L.pstride, 0, rawA);
  load_x(L.base, L.len, L.vstride, L.pstride, 1, rawB);

  // ---- the whole EPIConv.0 weight, rounded, once per block.  Source order (coalesced): i = (tap, n, eight-channel chunk kc = 4 ks + g) ----
  //      Four slots per thread and round trip (12.5 per thread in all): one at a time, the staging was thirteen dependent trips to L2 in front of the first MFMA ----
  for (int i0 = tid; i0 < EK_SLOTS; i0 += 4 * 512) {
    f32x4b lo[4], hi[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int i = i0 + 512 * k < EK_SLOTS ? i0 + 512 * k : EK_SLOTS - 1;      // (no branch around the loads: the slots past the end are dropped below)
      lo[k] = *reinterpret_cast<const f32x4b*>(p.W1 + i * 8); hi[k] = *reinterpret_cast<const f32x4b*>(p.W1 + i * 8 + 4);
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int i = i0 + 512 * k;
      const int kc = i & 7, n = (i >> 3) & 31, tap = i >> 8;
      const int dx = tap / 5, v = tap - 5 * dx, ks = kc >> 2, kg = kc & 3;
      if (i < EK_SLOTS) reinterpret_cast<u32x4b*>(sW)[((2 * v + ks) * 5 + dx) * 128 + kg * 32 + n] = bb_cvt8(lo[k], hi[k]);
    }
  }
#pragma unroll
  for (int nt = 0; nt < 2; ++nt) pA[nt] = bb_cvt8(rawA[nt][0], rawA[nt][1]);
  __syncthreads();
  const int aoff = (g * 32 + l15) * 16;                 // this lane's A-operand slot inside a dx block: k-group g, weight row l15 (+ 16 mt)

  for (;;) {
    const bool more = it + 1 < nunits;  // (block-uniform)
    const Line Ln = line_of(it + 1);    // (past the end: an absent line, every access out of range)
    f32x4b acc[5][2][2];
#pragma unroll
    for (int dx = 0; dx < 5; ++dx)
#pragma unroll
      for (int mt = 0; mt < 2; ++mt) { acc[dx][mt][0] = f32x4b{0.f, 0.f, 0.f, 0.f}; acc[dx][mt][1] = acc[dx][mt][0]; }
#pragma unroll
    for (int dx = 0; dx < 5; ++dx) asm volatile("s_nop 1" : "+v"(acc[dx][0][0]), "+v"(acc[dx][0][1]), "+v"(acc[dx][1][0]), "+v"(acc[dx][1][1]));

    // one step: MFMAs of step j on the operands u; raw values rs (step j + 1) converted into d; loads of step j + 2 into rd
    auto step = [&](int j, u32x4b (&u)[2], f32x4b (&rs)[2][2], u32x4b (&d)[2], f32x4b (&rd)[2][2]) {
      {                                 // (the line picked by selects: a branch here would put the loads behind it and cost the counted waits)
        const bool nl = j + 2 >= 10;
        load_x(nl ? Ln.base : L.base, nl ? Ln.len : L.len, nl ? Ln.vstride : L.vstride, nl ? Ln.pstride : L.pstride, nl ? j + 2 - 10 : j + 2, rd);
      }
      asm volatile("s_nop 4" : "+v"(u[0]), "+v"(u[1]));
      const unsigned char* wb = sW + j * EK_STEP_BYTES + aoff;
      u32x4b af[2][2];                  // A operands (tap dx, row tile mt) one group ahead of their MFMAs
      auto load_a = [&](int dx, u32x4b (&a)[2]) {
#pragma unroll
        for (int mt = 0; mt < 2; ++mt) a[mt] = *reinterpret_cast<const u32x4b*>(wb + (dx * 128 + 16 * mt) * 16);
      };
      load_a(0, af[0]);
#pragma unroll
      for (int dx = 0; dx < 5; ++dx) {
        if (dx + 1 < 5) load_a(dx + 1, af[(dx + 1) & 1]);
        bb_mfma(acc[dx][0][0], af[dx & 1][0], u[0]);
        bb_mfma(acc[dx][0][1], af[dx & 1][0], u[1]);
        bb_mfma(acc[dx][1][0], af[dx & 1][1], u[0]);
        bb_mfma(acc[dx][1][1], af[dx & 1][1], u[1]);
        // the next step's conversion (8 VALU) as one burst, at a point of the step that differs between the two waves of a SIMD (as k_epi_b3's split)
        if (dx == (phase ? 3 : 0)) {
          asm volatile("" : "+v"(rs[0][0]), "+v"(rs[0][1]), "+v"(rs[1][0]), "+v"(rs[1][1]));
#pragma unroll
          for (int nt = 0; nt < 2; ++nt) d[nt] = bb_cvt8(rs[nt][0], rs[nt][1]);
          asm volatile("" : "+v"(d[0]), "+v"(d[1]));
        }
      }
    };
#pragma unroll 1
    for (int jj = 0; jj < 10; jj += 2) {
      step(jj, pA, rawB, pB, rawA);
      step(jj + 1, pB, rawA, pA, rawB);
    }

    // ---- t[x][n] = sum_dx Z_dx[n][x + dx - 2] (DPP row shifts, as k_epi_b3), LeakyReLU, store ----
#pragma unroll
    for (int dx = 0; dx < 5; ++dx)
      asm volatile("s_nop 15\n\ts_nop 15" : "+v"(acc[dx][0][0]), "+v"(acc[dx][0][1]), "+v"(acc[dx][1][0]), "+v"(acc[dx][1][1]));
    f32x4b tv[2][2];                    // [mt][nt]: channels 16 mt + 4 g .. + 3 of position 16 nt + l15
#pragma unroll
    for (int mt = 0; mt < 2; ++mt) {
      tv[mt][0] = acc[2][mt][0]; tv[mt][1] = acc[2][mt][1];
      ek_shift_add<-2>(tv[mt], acc[0][mt]);
      ek_shift_add<-1>(tv[mt], acc[1][mt]);
      ek_shift_add<1>(tv[mt], acc[3][mt]);
      ek_shift_add<2>(tv[mt], acc[4][mt]);
    }
#pragma unroll
    for (int nt = 0; nt < 2; ++nt) {
      const int pos = 16 * nt + l15;
      const int to = (L.base >= 0 && pos < L.len) ? ((L.row + pos * L.rowstep) * 32 + 4 * g) * 4 : EOOB;      // an absent row: out of range, the store is dropped
#pragma unroll
      for (int mt = 0; mt < 2; ++mt) {
        f32x4b z = tv[mt][nt];
#pragma unroll
        for (int r = 0; r < 4; ++r) z[r] = fmaxf(z[r], z[r] * p.slope);      // LeakyReLU, 0 <= slope <= 1 (checked by the launcher)
        const int o = to == EOOB ? EOOB : to + 64 * mt;
        // (both passes' stores issued, the other one out of range: no store behind a branch; the whole offset in the VGPR field)
        __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4b, z), rsH, L.vert ? EOOB : o, 0, 0);
        __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4b, z), rsV, L.vert ? o : EOOB, 0, 0);
        asm volatile("s_nop 1" : "+v"(z));      // (store data -> a later asm MFMA writing the same registers: k_epi_b3's store hazard)
      }
    }
    if (!more) break;
    ++it;
    L = Ln;
  }
}

// =====================================================================================================================================================
// block tail
// =====================================================================================================================================================
constexpr int BT_WAVES = 8;
constexpr int BT_BLOCKS_PER_CU = 2;
constexpr int BT_FBYTES = 64 * 160 * 2;              // fuse.0: [K step 5][k-group 4][row 64][8 bf16]: 20480
constexpr int BT_ESLOTS = 4 * 160;                   // EPIConv.2: [k-group][n' 160] 16-B slots
constexpr int BT_EBYTES = BT_ESLOTS * 16;            // 10240
constexpr int BT_AFLOATS = 25 * 16 * 16;             // AngConv.2, perm 1: [view * 16 + c][16], fp32
constexpr int BT_ABYTES = BT_AFLOATS * 4;            // 25600
constexpr int BT_CROW = 88;                          // concat tile row, bf16: ang 0..15 | epiH 16..47 | epiV 48..79 (+ 8 pad): 176 B
constexpr int BT_CBYTES = BT_WAVES * 16 * BT_CROW * 2;   // 22528
constexpr int BT_SMEM = BT_FBYTES + BT_EBYTES + BT_ABYTES + BT_CBYTES;   // 78848: two blocks in a CU's 160 KB

struct TailBf16Args {
  const float* S; int s_stride; int s_choff; int s_bytes;     // SpaConv.2 output, VCL
  const float* TA; int ta_bytes;                              // (B h w, 16)
  const float* TH; const float* TV; int te_bytes;             // (B A h w, 32) each
  const float* WA2;                                           // AngConv.2, perm-1 pack
  const float* WE2;                                           // EPIConv.2 direct pack, fp32: [n' 160][k 32]
  const float* WF;                                            // fuse.0, packed [64][144]
  float* Y; int y_stride; int y_choff; int y_bytes;           // T, VCL
  int B, H, W;
  float slope;
};

__global__ __launch_bounds__(512, BT_BLOCKS_PER_CU) void k_distg_tail_bf16(TailBf16Args p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  unsigned short* const sF = reinterpret_cast<unsigned short*>(smem_raw);
  unsigned char* const sE = smem_raw + BT_FBYTES;
  float* const sA = reinterpret_cast<float*>(smem_raw + BT_FBYTES + BT_EBYTES);
  unsigned short* const sC = reinterpret_cast<unsigned short*>(smem_raw + BT_FBYTES + BT_EBYTES + BT_ABYTES);
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

  // A tile's place in the three operands (k_distg_tail).  lane (l15, g): macro-pixel m = 16 tile + l15 -- the B-operand column of the bf16 MFMAs (and the A row of
  // the fp32 ones).  A tile past the end (a wave without work, the hand-over behind a wave's last tile) has no row in range: every load of it moves no data.
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
  auto tro = [&](const Tile& c, int q) { return c.ok ? ((c.tb + q * HW) * 32 + 4 * g) * 4 : EOOB; };      // t_H / t_V row (b, q, y, x): channels 4 g .. + 3 (+ 64 B: 16 + 4 g)
  auto pixo = [&](const Tile& c, int view) { return c.ok ? c.pb + view * HW : -1; };                       // VCL pixel of this lane's row in a view

  // raw operands of one view, double-buffered one body ahead; no load sits behind a run-time branch: a row that is not wanted gets an out-of-range offset
  f32x4b sr0[2][2], sr1[2][2], vr0[2], vr1[2], hr[2], a2n;
  auto load_view = [&](const Tile& c, int view, f32x4b (&sr)[2][2], f32x4b (&vr)[2]) {
    const int pix = pixo(c, view);
    const int so = pix >= 0 ? (pix * p.s_stride + p.s_choff + 8 * g) * 4 : EOOB;
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
      for (int e = 0; e < 2; ++e) sr[s][e] = __builtin_bit_cast(f32x4b, __builtin_amdgcn_raw_buffer_load_b128(rsS, so == EOOB ? EOOB : so + (32 * s + 4 * e) * 4, 0, 0));
    const int vo = tro(c, view % A);
    vr[0] = __builtin_bit_cast(f32x4b, __builtin_amdgcn_raw_buffer_load_b128(rsV, vo, 0, 0));
    vr[1] = __builtin_bit_cast(f32x4b, __builtin_amdgcn_raw_buffer_load_b128(rsV, vo == EOOB ? EOOB : vo + 64, 0, 0));
  };
  auto load_h = [&](int ho) {
    hr[0] = __builtin_bit_cast(f32x4b, __builtin_amdgcn_raw_buffer_load_b128(rsH, ho, 0, 0));
    hr[1] = __builtin_bit_cast(f32x4b, __builtin_amdgcn_raw_buffer_load_b128(rsH, ho == EOOB ? EOOB : ho + 64, 0, 0));
  };
  auto load_first = [&](const Tile& c) {        // what a tile needs before its first view: t_A, view 0, t_H row 0
    a2n = __builtin_bit_cast(f32x4b, __builtin_amdgcn_raw_buffer_load_b128(rsA, c.ao, 0, 0));   // t_A row m, k = 4 g .. + 3
    load_view(c, 0, sr0, vr0);
    load_h(tro(c, 0));
  };

  // the wave's first tile is requested before the weights
  int tile = (int)blockIdx.x * BT_WAVES + wave;
  Tile nx = place(tile);
  load_first(nx);

  // ---- weights, once per block: rounded from the fp32 packs ----
  for (int i = tid; i < 64 * 20; i += 512) {       // fuse.0: KV = 144 of K = 160; columns >= 144 zero
    const int r = i / 20, c = i - r * 20;
    const bool ok = c * 8 < 144;
    const float* src = p.WF + r * 144 + (ok ? c * 8 : 0);
    f32x4b lo = *reinterpret_cast<const f32x4b*>(src), hi = *reinterpret_cast<const f32x4b*>(src + 4);
    if (!ok) { lo = f32x4b{0.f, 0.f, 0.f, 0.f}; hi = lo; }
    *reinterpret_cast<u32x4b*>(sF + (c * 64 + r) * 8) = bb_cvt8(lo, hi);
  }
  for (int i = tid; i < BT_ESLOTS; i += 512) {     // EPIConv.2: k slot 8 g + j <-> hidden channel 16 (j >> 2) + 4 g + (j & 3), the order of the t rows' loads
    const int n = i % 160, kg = i / 160;
    const f32x4b lo = *reinterpret_cast<const f32x4b*>(p.WE2 + n * 32 + 4 * kg), hi = *reinterpret_cast<const f32x4b*>(p.WE2 + n * 32 + 16 + 4 * kg);
    reinterpret_cast<u32x4b*>(sE)[i] = bb_cvt8(lo, hi);
  }
  for (int i = tid; i < BT_AFLOATS / 4; i += 512) reinterpret_cast<float4*>(sA)[i] = reinterpret_cast<const float4*>(p.WA2)[i];
  __syncthreads();

  unsigned short* const st = sC + wave * 16 * BT_CROW;                 // this wave's concat tile [row][BT_CROW]
  const unsigned char* const wE = sE + (g * 160 + l15) * 16;           // EPIConv.2 A operand: k-group g, row l15 (+ 16 per row tile)
  const unsigned short* const wF = sF + (g * 64 + l15) * 8;            // fuse.0 A operand: k-group g, row l15 (+ 16 rows per column tile, + 256 slots per K step)
  const float* const bA = sA + l15 * 16 + 4 * g;                       // AngConv.2 B operand (+ 256 per view)

  for (; tile < ntiles; tile += (int)gridDim.x * BT_WAVES) {
    const Tile cur = nx;
    const f32x4b a2 = a2n;
    u32x4b hp;                           // t_H (row u of the current view) as a B operand

    // LAST is a property of the body's copy, not of the view (k_distg_tail): the trailing body requests the first rows of the wave's next tile
    auto body = [&](int view, f32x4b (&sr)[2][2], f32x4b (&vr)[2], f32x4b (&srn)[2][2], f32x4b (&vrn)[2], auto last) {
      constexpr bool LAST = decltype(last)::value;
      const int u = view / A, v = view - A * u;
      const float4 b = *reinterpret_cast<const float4*>(bA + view * 256);      // AngConv.2 B operand
      if constexpr (LAST) a2n = __builtin_bit_cast(f32x4b, __builtin_amdgcn_raw_buffer_load_b128(rsA, nx.ao, 0, 0));
      else load_view(cur, view + 1, srn, vrn);
      if (v == 0) hp = bb_cvt8(hr[0], hr[1]);                          // (before the t_H request below: that one lands in hr)
      load_h(LAST ? tro(nx, 0) : v == A - 1 && u + 1 < A ? tro(cur, u + 1) : EOOB);      // row u + 1 during the last view of row u; nothing otherwise
      // EPIConv.2 A operands, one group ahead: horizontal = chunk v of t_H (row u), vertical = chunk u of t_V (column v)
      u32x4b aH[2], aV[2];
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        aH[h] = *reinterpret_cast<const u32x4b*>(wE + 16 * (2 * v + h) * 16);
        aV[h] = *reinterpret_cast<const u32x4b*>(wE + 16 * (2 * u + h) * 16);
      }
      // ---- AngConv.2 of this view (k_ang_fused stage 2, fp32 MFMA): D[macro-pixel 4 g + r][channel l15] ----
      {
        f32x4b o = {0.f, 0.f, 0.f, 0.f};
        o = __builtin_amdgcn_mfma_f32_16x16x4f32(a2.x, b.x, o, 0, 0, 0);
        o = __builtin_amdgcn_mfma_f32_16x16x4f32(a2.y, b.y, o, 0, 0, 0);
        o = __builtin_amdgcn_mfma_f32_16x16x4f32(a2.z, b.z, o, 0, 0, 0);
        o = __builtin_amdgcn_mfma_f32_16x16x4f32(a2.w, b.w, o, 0, 0, 0);
        float z[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) z[r] = o[r] >= 0.f ? o[r] : o[r] * p.slope;
        const unsigned q01 = bb_cvt_pk(z[0], z[1]), q23 = bb_cvt_pk(z[2], z[3]);
        st[(4 * g + 0) * BT_CROW + l15] = (unsigned short)(q01 & 0xffffu);
        st[(4 * g + 1) * BT_CROW + l15] = (unsigned short)(q01 >> 16);
        st[(4 * g + 2) * BT_CROW + l15] = (unsigned short)(q23 & 0xffffu);
        st[(4 * g + 3) * BT_CROW + l15] = (unsigned short)(q23 >> 16);
      }

      // ---- EPIConv.2 of both passes: one product per accumulator ----
      {
        u32x4b vp = bb_cvt8(vr[0], vr[1]);
        asm volatile("s_nop 4" : "+v"(hp), "+v"(vp));
        f32x4b e[2][2];                  // [pass][row tile h]: channels 16 h + 4 g + r of macro-pixel l15
#pragma unroll
        for (int i = 0; i < 2; ++i) { e[i][0] = f32x4b{0.f, 0.f, 0.f, 0.f}; e[i][1] = e[i][0]; }
        asm volatile("s_nop 1" : "+v"(e[0][0]), "+v"(e[0][1]), "+v"(e[1][0]), "+v"(e[1][1]));
        bb_mfma(e[0][0], aH[0], hp); bb_mfma(e[1][0], aV[0], vp);
        bb_mfma(e[0][1], aH[1], hp); bb_mfma(e[1][1], aV[1], vp);
        asm volatile("s_nop 15\n\ts_nop 15" : "+v"(e[0][0]), "+v"(e[0][1]), "+v"(e[1][0]), "+v"(e[1][1]));
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
          for (int h = 0; h < 2; ++h) {
            f32x4b z = e[i][h];
#pragma unroll
            for (int r = 0; r < 4; ++r) z[r] = fmaxf(z[r], z[r] * p.slope);
            *reinterpret_cast<u32x2b*>(st + l15 * BT_CROW + 16 + 32 * i + 16 * h + 4 * g) = u32x2b{bb_cvt_pk(z[0], z[1]), bb_cvt_pk(z[2], z[3])};
          }
      }
      __builtin_amdgcn_wave_barrier();

      // ---- fuse.0: B operand = row l15, channels 32 s + 8 g .. + 7; K steps 0, 1 the SpaConv.2 row, 2 .. 4 the concat tile (rounded when it was written) ----
      u32x4b wa[2][2];                   // fuse.0 A operands of group gi = 2 s + t / 2 (K step s, column tiles t, t + 1), double-buffered
      auto load_wf = [&](int gi) {
        const int s = gi >> 1, t = 2 * (gi & 1);
        wa[gi & 1][0] = *reinterpret_cast<const u32x4b*>(wF + (4 * s * 64 + t * 16) * 8);
        wa[gi & 1][1] = *reinterpret_cast<const u32x4b*>(wF + (4 * s * 64 + (t + 1) * 16) * 8);
      };
      load_wf(0);
      u32x4b x[5];
#pragma unroll
      for (int s = 0; s < 2; ++s) x[s] = bb_cvt8(sr[s][0], sr[s][1]);
#pragma unroll
      for (int s = 2; s < 5; ++s) {
        const int gg = s == 4 ? (g & 1) : g;                            // channels 144 .. 159 do not exist: a valid address, then zero operand columns
        x[s] = *reinterpret_cast<const u32x4b*>(st + l15 * BT_CROW + 32 * (s - 2) + 8 * gg);
        if (s == 4 && g >= 2) x[s] = u32x4b{0u, 0u, 0u, 0u};
      }
      __builtin_amdgcn_wave_barrier();
      f32x4b acc[4];
#pragma unroll
      for (int t = 0; t < 4; ++t) acc[t] = f32x4b{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int s = 0; s < 5; ++s) asm volatile("s_nop 4" : "+v"(x[s]));
      asm volatile("s_nop 1" : "+v"(acc[0]), "+v"(acc[1]), "+v"(acc[2]), "+v"(acc[3]));
      if constexpr (LAST) load_view(nx, 0, sr, vr);      // 25 views: the next tile starts in the set this view has just converted
#pragma unroll
      for (int gi = 0; gi < 10; ++gi) {
        const int s = gi >> 1, t = 2 * (gi & 1);
        if (gi + 1 < 10) load_wf(gi + 1);
        bb_mfma(acc[t], wa[gi & 1][0], x[s]);
        bb_mfma(acc[t + 1], wa[gi & 1][1], x[s]);
      }
      asm volatile("s_nop 15\n\ts_nop 15" : "+v"(acc[0]), "+v"(acc[1]), "+v"(acc[2]), "+v"(acc[3]));
      const int pix = pixo(cur, view);
      const int yo = pix >= 0 ? (pix * p.y_stride + p.y_choff + 4 * g) * 4 : EOOB;
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        f32x4b z = acc[t];
#pragma unroll
        for (int r = 0; r < 4; ++r) z[r] = z[r] >= 0.f ? z[r] : z[r] * p.slope;
        __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4b, z), rsY, yo == EOOB ? EOOB : yo + 64 * t, 0, 0);
        asm volatile("s_nop 1" : "+v"(z));      // (store data -> a later asm MFMA writing the same registers: k_epi_b3's store hazard)
      }
    };
#pragma unroll 1
    for (int view = 0; view < AA - 1; view += 2) {
      body(view, sr0, vr0, sr1, vr1, std::false_type{});
      body(view + 1, sr1, vr1, sr0, vr0, std::false_type{});
    }
    nx = place(tile + (int)gridDim.x * BT_WAVES);
    body(AA - 1, sr0, vr0, sr1, vr1, std::true_type{});
  }
}

int device_cus(int& cus_out) {
  static std::atomic<bool> attr_set[64];
  static std::atomic<int> cus[64];
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return LFSR_HIP_ERR(hipErrorInvalidDevice);
  if (!attr_set[dev]) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(k_epi_bf16), hipFuncAttributeMaxDynamicSharedMemorySize, EK_SMEM);
    if (e == hipSuccess) e = hipFuncSetAttribute(reinterpret_cast<const void*>(k_distg_tail_bf16), hipFuncAttributeMaxDynamicSharedMemorySize, BT_SMEM);
    if (e != hipSuccess) return LFSR_HIP_ERR(e);
    int v = 0;
    cus[dev] = (hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && v > 0) ? v : 256;
    attr_set[dev] = true;
  }
  cus_out = cus[dev];
  return LFSR_OK;
}

}  // namespace

// Stage 1 of both EPI passes on bf16 operands (e.y null, which = 3): t_h, t_v written as lfsr_epi_b3_launch writes them for the same call.  Reads the fp32 direct
// pack of EPIConv.0.  LFSR_E_ARG = not covered, nothing launched (the dispatcher keeps lfsr_epi_b3_launch).
int lfsr_epi_bf16_launch(const LfsrEpi& e, hipStream_t st) {
  const int B = e.B, A = e.A, h = e.h, w = e.w;
  if (e.y || e.which != 3) return LFSR_E_ARG;
  if (A != 5 || h > 32 || w > 32 || h <= 0 || w <= 0 || B <= 0 || !e.x || !e.w0 || !e.t_h || !e.t_v) return LFSR_E_ARG;
  if ((e.x_stride | e.x_choff) & 3 || e.x_stride < e.x_choff + 64) return LFSR_E_ARG;
  if (((uintptr_t)e.x | (uintptr_t)e.w0 | (uintptr_t)e.t_h | (uintptr_t)e.t_v) & 15) return LFSR_E_ARG;
  if ((long long)B * A * A * h * w * e.x_stride * 4 >= (1LL << 31) || (long long)B * A * h * w * 32 * 4 >= (1LL << 31)) return LFSR_E_ARG;   // 32-bit byte offsets
  if (!(e.slope >= 0.f && e.slope <= 1.f)) return LFSR_E_ARG;      // LeakyReLU as max(v, slope v)
  int cus = 0;
  LFSR_RC(device_cus(cus));
  EpiBf16Args p{};
  p.X = e.x; p.x_stride = e.x_stride; p.x_choff = e.x_choff; p.x_bytes = (int)((long long)B * A * A * h * w * e.x_stride * 4);
  p.W1 = e.w0_direct(); p.TH = e.t_h; p.TV = e.t_v; p.te_bytes = (int)((long long)B * A * h * w * 32 * 4);
  p.B = B; p.H = h; p.W = w; p.slope = e.slope;
  p.tilesH = (B * A * h + EK_LINES - 1) / EK_LINES;
  p.tilesV = (B * A * w + EK_LINES - 1) / EK_LINES;
  const int ngroups = p.tilesH + p.tilesV;
  if ((A * h) % EK_LINES == 0 && (A * w) % EK_LINES == 0) { p.tpiH = A * h / EK_LINES; p.tpiV = A * w / EK_LINES; }
  const int grid = cus < ngroups ? cus : ngroups;
  hipLaunchKernelGGL(k_epi_bf16, dim3((unsigned)grid), dim3(512), EK_SMEM, st, p);
  LFSR_CHECK_LAUNCH();
  return LFSR_OK;
}

// The block tail on bf16 operands: lfsr_distg_tail_launch's call, reading the fp32 direct pack of EPIConv.2 ([160][32]), not its planes.
// LFSR_E_ARG = not covered, nothing launched (the dispatcher keeps lfsr_distg_tail_launch).
int lfsr_distg_tail_bf16_launch(const LfsrDistgTail& t, hipStream_t st) {
  const int B = t.B, A = t.A, h = t.h, w = t.w;
  if (A != 5 || B <= 0 || h <= 0 || w <= 0 || !t.spa || !t.t_a || !t.t_h || !t.t_v || !t.w_ang2 || !t.w_epi2 || !t.w_fuse0 || !t.y) return LFSR_E_ARG;
  if ((t.spa_stride | t.spa_choff | t.y_stride | t.y_choff) & 3 || t.spa_stride < t.spa_choff + 64 || t.y_stride < t.y_choff + 64) return LFSR_E_ARG;
  if (((uintptr_t)t.spa | (uintptr_t)t.t_a | (uintptr_t)t.t_h | (uintptr_t)t.t_v | (uintptr_t)t.w_ang2 | (uintptr_t)t.w_epi2 | (uintptr_t)t.w_fuse0 | (uintptr_t)t.y) & 15)
    return LFSR_E_ARG;
  if (!(t.slope >= 0.f && t.slope <= 1.f)) return LFSR_E_ARG;      // LeakyReLU as max(v, slope v) in the epipolar stage
  const long long npix = (long long)B * A * A * h * w;
  if (npix * t.spa_stride * 4 >= (1LL << 31) || npix * t.y_stride * 4 >= (1LL << 31) || (long long)B * A * h * w * 32 * 4 >= (1LL << 31)) return LFSR_E_ARG;   // 32-bit byte offsets
  int cus = 0;
  LFSR_RC(device_cus(cus));
  TailBf16Args p{};
  p.S = t.spa; p.s_stride = t.spa_stride; p.s_choff = t.spa_choff; p.s_bytes = (int)(npix * t.spa_stride * 4);
  p.TA = t.t_a; p.ta_bytes = (int)((long long)B * h * w * 16 * 4);
  p.TH = t.t_h; p.TV = t.t_v; p.te_bytes = (int)((long long)B * A * h * w * 32 * 4);
  p.WA2 = t.w_ang2; p.WE2 = t.w_epi2_direct(); p.WF = t.w_fuse0;
  p.Y = t.y; p.y_stride = t.y_stride; p.y_choff = t.y_choff; p.y_bytes = (int)(npix * t.y_stride * 4);
  p.B = B; p.H = h; p.W = w; p.slope = t.slope;
  const long long ntiles = ((long long)B * h * w + 15) / 16;
  long long grid = (ntiles + BT_WAVES - 1) / BT_WAVES;
  if (grid > (long long)BT_BLOCKS_PER_CU * cus) grid = (long long)BT_BLOCKS_PER_CU * cus;
  hipLaunchKernelGGL(k_distg_tail_bf16, dim3((unsigned)grid), dim3(BT_WAVES * 64), BT_SMEM, st, p);
  LFSR_CHECK_LAUNCH();
  return LFSR_OK;
}
