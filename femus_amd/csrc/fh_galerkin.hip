// Galerkin coarse operator ELEMENT BY ELEMENT (uniform refinement): A = sum_e K_e and every fine element lies in one coarse element, whose
// 27 (9) nodes interpolate its nodes by the fixed child matrix C_j (the rows of the element prolongator, ElemType.cpp:439-532), so
//   PP^T KK PP = sum_E sum_{children j of E} C_j^T K_{child j} C_j          (LinearImplicitSystem.cpp:347-370, PetscMatrix.cpp:733-751)
// -- coarse ELEMENT matrices from the fine ones the assembler still holds, then the same row pass as the assembly.  The general sparse triple
// product streams ~10 elementary products per non-zero (8 ms on the 64^3 level); this reads the element-row buffer once (1.8 GB) and does
// 7 k multiply-adds per child with the 125 non-zeros of C_j.  Rows of the interpolation at fine Dirichlet nodes and its columns at coarse
// Dirichlet nodes are zero (ZeroInterpolatorDirichletNodes, :1032-1120): masks on K_j and on the result.  Same value as the product up to
// the order of the sums.  One wave per coarse element.
#include "fh_assembler.h"
#include "fh_fe.h"
#include <algorithm>

template <int NC, int NCH>
__global__ __launch_bounds__(256) void k_galerkin_elem(int nelc, const int* __restrict__ child, const int* __restrict__ slot_f, const double* __restrict__ Kf, int ks_f,
                                                       const int* __restrict__ edof_f, int nloc_f, const unsigned char* __restrict__ fb,
                                                       const int* __restrict__ slot_c, double* __restrict__ Kc, int ks_c, const int* __restrict__ edof_c, int nloc_c,
                                                       const unsigned char* __restrict__ cb, const unsigned char* __restrict__ tab_cnt,
                                                       const unsigned char* __restrict__ tab_row, const double* __restrict__ tab_val) {
  constexpr int NE = NC * NC, NT = (NE + 63) / 64, LD = NC + 1;
  __shared__ double cval[NCH * NC * 8];
  __shared__ unsigned char crow[NCH * NC * 8], ccnt[NCH * NC];
  __shared__ double slab[4][2][NC * LD];
  for (int k = threadIdx.x; k < NCH * NC * 8; k += 256) { cval[k] = tab_val[k]; crow[k] = tab_row[k]; }
  for (int k = threadIdx.x; k < NCH * NC; k += 256) ccnt[k] = tab_cnt[k];
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  double* Ks = slab[wave][0];
  double* Ts = slab[wave][1];
  for (int E = blockIdx.x * 4 + wave; E < nelc; E += gridDim.x * 4) {
    double acc[NT];
#pragma unroll
    for (int t = 0; t < NT; t++) acc[t] = 0.0;
    for (int j = 0; j < NCH; j++) {
      const int ej = child[(size_t)E * NCH + j];
      // all gathers of the child first (independent chains in flight), then the LDS writes
      double kin[NT];
#pragma unroll
      for (int t = 0; t < NT; t++) {
        const int idx = min(lane + 64 * t, NE - 1);
        const int i = idx / NC, c = idx - i * NC;
        const int s = slot_f[(size_t)ej * NC + i];
        const bool dead = s < 0 || fb[edof_f[(size_t)ej * nloc_f + i]] || fb[edof_f[(size_t)ej * nloc_f + c]];
        kin[t] = dead ? 0.0 : Kf[(size_t)max(s, 0) * ks_f + c];
      }
#pragma unroll
      for (int t = 0; t < NT; t++) {
        const int idx = lane + 64 * t;
        if (idx < NE) Ks[(idx / NC) * LD + idx % NC] = kin[t];
      }
      wave_lds_sync();
      // T = K_j C_j and K_E += C_j^T T: the (at most 8) non-zeros of a column of C_j, padded with zero weights -- a fixed trip count and
      // NT independent chains per lane instead of one serial chain of dependent LDS reads per entry
      {
        double tv[NT];
        int rbase[NT], cbase[NT];
#pragma unroll
        for (int t = 0; t < NT; t++) {
          const int idx = min(lane + 64 * t, NE - 1);
          rbase[t] = (idx / NC) * LD;
          cbase[t] = (j * NC + idx % NC) * 8;
          tv[t] = 0.0;
        }
#pragma unroll
        for (int q = 0; q < 8; q++)
#pragma unroll
          for (int t = 0; t < NT; t++) tv[t] += Ks[rbase[t] + crow[cbase[t] + q]] * cval[cbase[t] + q];
#pragma unroll
        for (int t = 0; t < NT; t++) {
          const int idx = lane + 64 * t;
          if (idx < NE) Ts[(idx / NC) * LD + idx % NC] = tv[t];
        }
      }
      wave_lds_sync();
      {
        int kcol[NT], abase[NT];
#pragma unroll
        for (int t = 0; t < NT; t++) {
          const int idx = min(lane + 64 * t, NE - 1);
          kcol[t] = idx % NC;
          abase[t] = (j * NC + idx / NC) * 8;
        }
#pragma unroll
        for (int q = 0; q < 8; q++)
#pragma unroll
          for (int t = 0; t < NT; t++) acc[t] += cval[abase[t] + q] * Ts[crow[abase[t] + q] * LD + kcol[t]];
      }
      wave_lds_sync();
    }
#pragma unroll
    for (int t = 0; t < NT; t++) {
      const int idx = lane + 64 * t;
      if (idx < NE) {
        const int a = idx / NC, k = idx - a * NC;
        const int s = slot_c[(size_t)E * NC + a];
        if (s >= 0) {
          const bool dead = cb[edof_c[(size_t)E * nloc_c + a]] || cb[edof_c[(size_t)E * nloc_c + k]];
          Kc[(size_t)s * ks_c + k] = dead ? 0.0 : acc[t];
        }
      }
    }
  }
}

// The same on the FP64 matrix cores (default): per child two small dense products T = K_j C_j and K_E += C_j^T T as v_mfma_f64_16x16x4 tiles
// (27 -> 32 x 32 x 28 padded: 2 x 28 instructions of 64 cycles), operands from LDS (the eight C_j, the gathered K_j, T), the element rows of
// the NEXT child gathered into registers while the current one is multiplied.  One wave per coarse element, one workgroup of four per CU.
// waves per workgroup: they share the child matrices C_j in LDS; the per-wave scratch holds K_j first and T = K_j C_j afterwards (one region), so that
// eight waves -- two per SIMD, one's LDS round trips behind the other's matrix instructions -- fit beside the 57 KB of C
constexpr int GAL_NW = 8;
template <int NC, int NCH>
__global__ __launch_bounds__(GAL_NW * 64) void k_galerkin_mfma(int nelc, const int* __restrict__ child, const int* __restrict__ slot_f, const double* __restrict__ Kf, int ks_f,
                                                       const int* __restrict__ edof_f, int nloc_f, const unsigned char* __restrict__ fb,
                                                       const int* __restrict__ slot_c, double* __restrict__ Kc, int ks_c, const int* __restrict__ edof_c, int nloc_c,
                                                       const unsigned char* __restrict__ cb, const double* __restrict__ Cdense /* [NCH][NC][NC] */) {
  constexpr int NE = NC * NC, NT = (NE + 63) / 64, MT = (NC + 15) / 16, KP = (NC + 3) / 4 * 4, CLD = MT * 16, KLD = KP + 1, TLD = MT * 16;
  extern __shared__ __attribute__((aligned(16))) double gm_smem[];
  double* Cs = gm_smem;                                   // [NCH][KP][CLD], zero padded
  for (int k = threadIdx.x; k < NCH * KP * CLD; k += GAL_NW * 64) {
    const int j = k / (KP * CLD), r = (k / CLD) % KP, c = k % CLD;
    Cs[k] = (r < NC && c < NC) ? Cdense[(j * NC + r) * NC + c] : 0.0;
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  constexpr int WS = (MT * 16 * KLD > KP * TLD) ? MT * 16 * KLD : KP * TLD;    // doubles of scratch per wave
  double* Ks = Cs + NCH * KP * CLD + wave * WS;      // [MT*16][KLD]
  double* Ts = Ks;                                    // [KP][TLD]: the same region, after K_j has been consumed
  __syncthreads();
  const int kk = lane >> 4, li = lane & 15;
  typedef double d4 __attribute__((ext_vector_type(4)));
  for (int E = blockIdx.x * GAL_NW + wave; E < nelc; E += gridDim.x * GAL_NW) {
    d4 KE[MT][MT];
#pragma unroll
    for (int a = 0; a < MT; a++)
#pragma unroll
      for (int b = 0; b < MT; b++) KE[a][b] = d4{0.0, 0.0, 0.0, 0.0};
    double kin[NT];
    auto gather = [&](int j) {      // K_j with the rows / columns of Dirichlet nodes zeroed (kept in registers until the LDS is free)
      const int ej = child[(size_t)E * NCH + j];
      const int ln = min(lane, NC - 1);
      const int sl = slot_f[(size_t)ej * NC + ln];
      const bool dn = sl < 0 || fb[edof_f[(size_t)ej * nloc_f + ln]];
      const unsigned long long dead = __ballot(dn && lane < NC);
#pragma unroll
      for (int t = 0; t < NT; t++) {
        const int idx = min(lane + 64 * t, NE - 1);
        const int i = idx / NC, c = idx - i * NC;
        const int s = __shfl(sl, i, 64);
        const bool d = ((dead >> i) | (dead >> c)) & 1ull;
        kin[t] = d ? 0.0 : Kf[(size_t)max(s, 0) * ks_f + c];
      }
    };
    gather(0);
    for (int j = 0; j < NCH; j++) {
#pragma unroll
      for (int t = 0; t < NT; t++) {
        const int idx = lane + 64 * t;
        if (idx < NE) Ks[(idx / NC) * KLD + idx % NC] = kin[t];
      }
      // the padding of K_j (rows and columns NC .. of the operand tile) is zero: T of the previous child lived here
      for (int q = lane; q < (MT * 16 - NC) * KLD; q += 64) Ks[NC * KLD + q] = 0.0;
      for (int q = lane; q < NC * (KLD - NC); q += 64) Ks[(q / (KLD - NC)) * KLD + NC + q % (KLD - NC)] = 0.0;
      wave_lds_sync();
      if (j + 1 < NCH) gather(j + 1);
      const double* Cj = Cs + j * KP * CLD;
      d4 T[MT][MT];
#pragma unroll
      for (int a = 0; a < MT; a++)
#pragma unroll
        for (int b = 0; b < MT; b++) T[a][b] = d4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
      for (int k0 = 0; k0 < KP; k0 += 4) {
        double av[MT], bv[MT];
#pragma unroll
        for (int x = 0; x < MT; x++) {
          av[x] = Ks[(x * 16 + li) * KLD + k0 + kk];
          bv[x] = Cj[(k0 + kk) * CLD + x * 16 + li];
        }
#pragma unroll
        for (int a = 0; a < MT; a++)
#pragma unroll
          for (int b = 0; b < MT; b++) T[a][b] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[a], bv[b], T[a][b], 0, 0, 0);
      }
      wave_lds_sync();                       // every lane has read its operands of K_j: T may take the region
#pragma unroll
      for (int a = 0; a < MT; a++)
#pragma unroll
        for (int r = 0; r < 4; r++) {
          const int i = a * 16 + kk + 4 * r;
          if (i < KP) {
#pragma unroll
            for (int b = 0; b < MT; b++) Ts[i * TLD + b * 16 + li] = T[a][b][r];
          }
        }
      wave_lds_sync();
#pragma unroll
      for (int k0 = 0; k0 < KP; k0 += 4) {
        double av[MT], bv[MT];
#pragma unroll
        for (int x = 0; x < MT; x++) {
          av[x] = Cj[(k0 + kk) * CLD + x * 16 + li];        // A[row a][k i] = C_j[i][a]
          bv[x] = Ts[(k0 + kk) * TLD + x * 16 + li];
        }
#pragma unroll
        for (int a = 0; a < MT; a++)
#pragma unroll
          for (int b = 0; b < MT; b++) KE[a][b] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[a], bv[b], KE[a][b], 0, 0, 0);
      }
      wave_lds_sync();
    }
    // rows / columns of coarse Dirichlet nodes are zero; rows without a slot are not stored
    const int ln = min(lane, NC - 1);
    const int slc = slot_c[(size_t)E * NC + ln];
    const unsigned long long cdead = __ballot(lane < NC && cb[edof_c[(size_t)E * nloc_c + ln]]);
#pragma unroll
    for (int a = 0; a < MT; a++)
#pragma unroll
      for (int r = 0; r < 4; r++) {
        const int ra = a * 16 + kk + 4 * r;
        const int s = __shfl(slc, min(ra, NC - 1), 64);
#pragma unroll
        for (int b = 0; b < MT; b++) {
          const int k = b * 16 + li;
          if (ra < NC && k < NC && s >= 0) {
            const bool d = ((cdead >> ra) | (cdead >> k)) & 1ull;
            Kc[(size_t)s * ks_c + k] = d ? 0.0 : KE[a][b][r];
          }
        }
      }
  }
}

template <int NC, int NCH>
static size_t galerkin_mfma_lds() {
  constexpr int MT = (NC + 15) / 16, KP = (NC + 3) / 4 * 4;
  const size_t ws = std::max((size_t)MT * 16 * (KP + 1), (size_t)KP * MT * 16);
  return ((size_t)NCH * KP * MT * 16 + GAL_NW * ws) * sizeof(double);
}

// ------------------------------------------------------------------------------------------------------------------
// Element-wise Galerkin product FROM THE MACRO ROWS of a fused assembly (round 5).  The fused path keeps no element rows; what it leaves behind per cluster
// (= per coarse element) is the 125 x 125 macro matrix K_m = sum_j S_j^T K_j S_j: complete rows in the CSR array, the others as packed rows in the
// partial-row buffer, 4913 entries at the addresses the cluster kernel stored them to.  With C (125 x 27) the interpolation from the coarse element,
// K_E = C^T K_m C = sum_j C_j^T K~_j C_j for ANY split of the macro entries over the children (K~_j = the entries child j owns: an entry met by several
// children belongs to the first, table gtab).  One workgroup of eight waves per coarse element: all threads read the 4913 entries back (the loads of the
// NEXT cluster fly during the products) into a template-ordered LDS array, wave j forms K~_j from it and runs the two 32 x 32 x 28 products of
// k_galerkin_mfma on the matrix cores, the eight results are added in child order and leave as coarse element rows.  39 kB read per coarse element instead
// of 55 kB, and the fused assembly stays the path of every assembly of a solve (LinearImplicitSystem.cpp:288-411: assemble -> Galerkin -> solve, every time).
// Between the assembly and this product only Dirichlet ROWS of the fine matrix may have been replaced (SetPenalty): they are masked here anyway.
// ------------------------------------------------------------------------------------------------------------------
constexpr int GMAC_NW = 8, GMAC_T = GMAC_NW * 64;
constexpr int GMAC_KP = 28;                                             // K of the two products, padded to the matrix instruction's 4
constexpr int GMAC_TN = 4928;                                           // template entries (4913), padded
constexpr int GMAC_RS = 27 * 28;                                        // one wave's result [27][28]
constexpr int GMAC_BUF = GMAC_NW * GMAC_RS > GMAC_TN ? GMAC_NW * GMAC_RS : GMAC_TN;      // the macro matrix, then the eight results (same region)
constexpr size_t gmac_lds_bytes() { return (size_t)GMAC_BUF * sizeof(double) + CL_NM_MAX * sizeof(unsigned long long) + 32 * sizeof(int); }
static_assert(gmac_lds_bytes() <= 160 * 1024, "k_galerkin_macro: LDS budget");

// Operands in registers (second form of the round; the first staged K~_j, C_j and T through LDS like k_galerkin_mfma and took 1.0 ms against that kernel's
// 0.86): wave j always serves child j, so its fragments of C_j -- B operand of T = K~_j C_j AND A operand of R = C_j^T T, the same values -- and the
// template indices of its K~_j fragments are loop invariant (14 doubles + 14 indices per lane); T leaves the first product in exactly the lanes the second
// product wants it as B operand (row 4 m + kk of T = accumulator m / 4, register m % 4 of lane (kk, li)): no LDS round trip between the two products.
// Dirichlet masks of the children's and of the coarse element's 27 nodes (bit = local node), once per hierarchy: the product kernel then needs no chain
// of dependent look-ups (children -> element dofs -> flags) per cluster
__global__ __launch_bounds__(256) void k_gal_masks(int nelc, const int* __restrict__ child, const int* __restrict__ edof_f, int nloc_f, const unsigned char* __restrict__ fb,
                                                    const int* __restrict__ edof_c, int nloc_c, const unsigned char* __restrict__ cb, unsigned* __restrict__ fmask,
                                                    unsigned* __restrict__ cmask) {
  const int k = blockIdx.x * 256 + threadIdx.x;
  if (k >= nelc * 9) return;
  const int E = k / 9, j = k % 9;
  unsigned m = 0;
  if (j < 8) {
    const int ej = child[(size_t)E * 8 + j];
    for (int n = 0; n < 27; n++) m |= (fb[edof_f[(size_t)ej * nloc_f + n]] ? 1u : 0u) << n;
    fmask[(size_t)E * 8 + j] = m;
  } else {
    for (int n = 0; n < 27; n++) m |= (cb[edof_c[(size_t)E * nloc_c + n]] ? 1u : 0u) << n;
    cmask[E] = m;
  }
}

template <bool INS>
__global__ __launch_bounds__(GMAC_T) void k_galerkin_macro(int nelc, const int* __restrict__ child, int nm, const unsigned* __restrict__ sinfo, const uint4* __restrict__ map,
                                                           const unsigned long long* __restrict__ vdst, const unsigned short* __restrict__ gtab,
                                                           const unsigned* __restrict__ fmask, const unsigned* __restrict__ cmask,
                                                           const int* __restrict__ slot_c, double* __restrict__ Kc, int ks_c, const double* __restrict__ Cdense /* [8][27][27] */,
                                                           unsigned long long* __restrict__ stamps) {
  constexpr int NC = 27, NCH = 8, NE = NC * NC, MT = 2, NK = GMAC_KP / 4;
  SfStamps st;
  if (INS) {
#pragma unroll
    for (int k = 0; k < 16; k++) st.acc[k] = 0;
  }
  extern __shared__ __attribute__((aligned(16))) double gmac_smem[];
  double* Tm = gmac_smem;                                 // the macro matrix in template order; behind the products: the eight results
  unsigned long long* rbl = reinterpret_cast<unsigned long long*>(gmac_smem + GMAC_BUF);
  int* slds = reinterpret_cast<int*>(rbl + CL_NM_MAX);    // slots of the coarse element's 27 rows
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int kk = lane >> 4, li = lane & 15;
  unsigned si[CL_SPT];
#pragma unroll
  for (int i = 0; i < CL_SPT; i++) si[i] = sinfo[i * CL_T + tid];
  // loop-invariant fragments of child `wave`: C_j[4 m + kk][16 x + li] and the template index of K~_j[16 x + li][4 m + kk]
  double creg[NK][MT];
  int gidx[NK][MT];
#pragma unroll
  for (int m = 0; m < NK; m++)
#pragma unroll
    for (int x = 0; x < MT; x++) {
      const int r = 4 * m + kk, c = x * 16 + li;
      creg[m][x] = (r < NC && c < NC) ? Cdense[((size_t)wave * NC + r) * NC + c] : 0.0;
      const unsigned short g = (c < NC && r < NC) ? gtab[(size_t)wave * NE + c * NC + r] : (unsigned short)0xffff;
      gidx[m][x] = g == 0xffff ? -1 : (int)g;
    }
  typedef double d4 __attribute__((ext_vector_type(4)));
  const int stride = gridDim.x;
  int E = blockIdx.x;
  if (E >= nelc) return;
  // pipeline: values of cluster n in registers (tv), map / destinations of cluster n + 1 in registers (mp, vd)
  const int tm = tid & (CL_NM_MAX - 1);
  int cl = child[(size_t)E * NCH] >> 3;
  if (tid < CL_NM_MAX) rbl[tid] = vdst[(size_t)cl * CL_NM_MAX + tm];
  uint4 mp = map[(size_t)cl * CL_T + tid];
  __syncthreads();
  double tv[CL_SPT];
  // where slot i of a cluster's macro matrix is read: position p of the row (complete / partial rows), or -- a row carried in the CSR array across the clusters of a
  // super-cluster (class bit 10 + i of word 3) -- the CSR position the map byte names, and only in the cluster that made the LAST contribution (bit i of word 3
  // clear; the entry holds the sum of all of them there; the pseudo child matrices still add up to the assembled matrix, which is all the coarse operator depends
  // on); -1: nothing to read
  auto slot_pos = [&](const uint4& q4, int i) {
    const unsigned mq[4] = {q4.x, q4.y, q4.z, q4.w};
    const int r = si[i] & 127, p = (si[i] >> 7) & 127;
    if (r >= nm) return -1;
    if ((mq[3] >> i) & 1u) return -1;
    return ((mq[3] >> (10 + i)) & 1u) ? (int)((mq[i >> 2] >> (8 * (i & 3))) & 255) : p;
  };
#pragma unroll
  for (int i = 0; i < CL_SPT; i++) {
    const int r = si[i] & 127, pos = slot_pos(mp, i);
    tv[i] = pos >= 0 ? reinterpret_cast<const double*>(rbl[r])[pos] : 0.0;
  }
  int En = min(E + stride, nelc - 1);
  int cln = child[(size_t)En * NCH] >> 3;
  unsigned long long vdn = vdst[(size_t)cln * CL_NM_MAX + tm];
  uint4 mpn = map[(size_t)cln * CL_T + tid];
  const int ln = min(lane, NC - 1);
  unsigned dmask = fmask[(size_t)E * NCH + wave], cdm = cmask[E];      // Dirichlet nodes of this wave's child / of the coarse element (k_gal_masks)
  int slc = slot_c[(size_t)E * NC + ln];
  if (INS) st.prev = __builtin_amdgcn_s_memtime();
  int ndone = 0;
#pragma unroll 1
  for (; E < nelc; E += stride) {
    sf_stamp<INS>(st, 0);
    // ---- the macro matrix of this cluster into LDS (template order); destinations of the next cluster into rbl ----
    {
      const unsigned mw[4] = {mp.x, mp.y, mp.z, mp.w};
#pragma unroll
      for (int i = 0; i < CL_SPT; i++) {
        const int r = si[i] & 127, mb = (mw[i >> 2] >> (8 * (i & 3))) & 255;
        const int j = ((mw[3] >> (10 + i)) & 1u) ? (int)((si[i] >> 7) & 127) : mb;      // carried row: the entry is p
        if (r < nm) Tm[(si[i] >> 14) + j] = tv[i];
      }
    }
    if (tid < CL_NM_MAX) rbl[tid] = vdn;      // (the loads through the previous content were issued one iteration ago and have landed in tv)
    if (tid < NC) slds[tid] = slc;
    sf_stamp<INS>(st, 1);
    __syncthreads();
    sf_stamp<INS>(st, 2);
    // the NEXT cluster's values: in flight during the products below
    mp = mpn;
#pragma unroll
    for (int i = 0; i < CL_SPT; i++) {
      const int r = si[i] & 127, pos = slot_pos(mp, i);
      tv[i] = pos >= 0 ? reinterpret_cast<const double*>(rbl[r])[pos] : 0.0;
    }
    {
      const int Enn = min(E + 2 * stride, nelc - 1);
      const int clnn = child[(size_t)Enn * NCH] >> 3;
      vdn = vdst[(size_t)clnn * CL_NM_MAX + tm];
      mpn = map[(size_t)clnn * CL_T + tid];
    }
    const unsigned long long cdead = cdm, dead = dmask;
    {   // the next element's masks and slots (consumed one iteration later)
      const int En1 = min(E + stride, nelc - 1);
      dmask = fmask[(size_t)En1 * NCH + wave];
      cdm = cmask[En1];
      slc = slot_c[(size_t)En1 * NC + ln];
    }
    sf_stamp<INS>(st, 3);
    // ---- wave j: T = K~_j C_j (A operand gathered from the macro matrix, rows / columns of Dirichlet nodes zeroed), R_j = C_j^T T ----
    d4 T[MT][MT], KE[MT][MT];
#pragma unroll
    for (int a = 0; a < MT; a++)
#pragma unroll
      for (int b = 0; b < MT; b++) { T[a][b] = d4{0.0, 0.0, 0.0, 0.0}; KE[a][b] = d4{0.0, 0.0, 0.0, 0.0}; }
    {
      double av[2][MT];                      // fragments of K~_j, one k-step ahead of the products
      auto gather = [&](int m, double (&o)[MT]) {
#pragma unroll
        for (int x = 0; x < MT; x++) {
          const int row = x * 16 + li, col = 4 * m + kk;
          const bool d = gidx[m][x] < 0 || (((dead >> min(row, 63)) | (dead >> min(col, 63))) & 1ull);
          const double v = Tm[max(gidx[m][x], 0)];
          o[x] = d ? 0.0 : v;
        }
      };
      gather(0, av[0]);
#pragma unroll
      for (int m = 0; m < NK; m++) {
        if (m + 1 < NK) gather(m + 1, av[(m + 1) & 1]);
#pragma unroll
        for (int a = 0; a < MT; a++)
#pragma unroll
          for (int b = 0; b < MT; b++) T[a][b] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[m & 1][a], creg[m][b], T[a][b], 0, 0, 0);
      }
    }
#pragma unroll
    for (int m = 0; m < NK; m++)
#pragma unroll
      for (int a = 0; a < MT; a++)
#pragma unroll
        for (int b = 0; b < MT; b++) KE[a][b] = __builtin_amdgcn_mfma_f64_16x16x4f64(creg[m][a], T[m / 4][b][m % 4], KE[a][b], 0, 0, 0);
    if (INS) {
      asm volatile("" ::"v"(KE[0][0][0]), "v"(KE[1][1][3]));
      sf_stamp<INS>(st, 4);
    }
    __syncthreads();                       // every wave is done with the macro matrix: the results take the region
    sf_stamp<INS>(st, 5);
    {
      double* Rs = Tm + wave * GMAC_RS;
#pragma unroll
      for (int a = 0; a < MT; a++)
#pragma unroll
        for (int r = 0; r < 4; r++) {
          const int ra = a * 16 + kk + 4 * r;
#pragma unroll
          for (int b = 0; b < MT; b++) {
            const int k = b * 16 + li;
            if (ra < NC && k < NC) Rs[ra * 28 + k] = KE[a][b][r];
          }
        }
    }
    sf_stamp<INS>(st, 6);
    __syncthreads();
    sf_stamp<INS>(st, 7);
    // ---- the eight results added in child order; rows / columns of coarse Dirichlet nodes are zero; rows without a slot are not stored ----
    for (int idx = tid; idx < NE; idx += GMAC_T) {
      const int i = idx / NC, k = idx - i * NC;
      double v = Tm[i * 28 + k];
#pragma unroll
      for (int w = 1; w < GMAC_NW; w++) v += Tm[w * GMAC_RS + i * 28 + k];
      const int s2 = slds[i];
      const bool d = ((cdead >> i) | (cdead >> k)) & 1ull;
      if (s2 >= 0) Kc[(size_t)s2 * ks_c + k] = d ? 0.0 : v;
    }
    sf_stamp<INS>(st, 8);
    __syncthreads();                       // the region is the next cluster's macro matrix
    sf_stamp<INS>(st, 9);
    ndone++;
  }
  if (INS && stamps && lane == 0) {
    unsigned long long* o = stamps + ((size_t)blockIdx.x * GMAC_NW + wave) * 20;
#pragma unroll
    for (int k = 0; k < 16; k++) o[k] = st.acc[k];
    o[16] = (unsigned long long)ndone;
  }
}

void GalerkinState::release() {
  for (void* q : {(void*)d_child, (void*)d_cnt, (void*)d_row, (void*)d_fb, (void*)d_cb, (void*)d_fmask, (void*)d_val, (void*)d_res, (void*)d_dense})
    if (q) hipFree(q);
  *this = GalerkinState();
}

// a table of the product on the device, in place of the one *d held (synchronous: once per hierarchy)
template <class T>
static int gal_upload(T** d, const void* h, size_t bytes) {
  if (*d) FH_CHECK_HIP(hipFree(*d));
  FH_CHECK_HIP(hipMalloc(d, bytes ? bytes : 8));
  if (bytes) FH_CHECK_HIP(hipMemcpy(*d, h, bytes, hipMemcpyHostToDevice));
  return 0;
}

extern "C" int fh_assembler_galerkin(fh_assembler_t fas, fh_assembler_t cas, const int* child, int nfb, const int* fbdc, int ncb, const int* cbdc, fh_mat_t Ac) {
  FH_GUARD_BEGIN
  FH_REQUIRE(fas && cas && child && Ac && (nfb == 0 || fbdc) && (ncb == 0 || cbdc), "fh_assembler_galerkin: null argument");
  FH_REQUIRE(fas->two_pass && cas->two_pass && fas->nc == cas->nc && fas->geom == cas->geom && (fas->nc == 27 || fas->nc == 9),
             "fh_assembler_galerkin: both levels need the two-pass biquadratic assembler");
  const int nch = fhfe::nvert_of(cas->geom), nc = cas->nc;
  FH_REQUIRE(fas->nel == cas->nel * nch, "fh_assembler_galerkin: %d fine elements are not the uniform refinement of %d coarse ones", fas->nel, cas->nel);
  FH_REQUIRE(Ac->m == cas->ndof, "fh_assembler_galerkin: the coarse matrix does not belong to the coarse assembler");
  fh_ctx_t c = cas->ctx;
  GalerkinState& G = cas->gal;
  // integer / table set-up, once per hierarchy -- and again when the children or the Dirichlet sets differ from the ones the tables were made from
  uint64_t key = 1469598103934665603ull;
  {
    auto mix = [&](const int* a, size_t n) {
      key = (key ^ (uint64_t)n) * 1099511628211ull;
      for (size_t k = 0; k < n; k++) key = (key ^ (uint64_t)(uint32_t)a[k]) * 1099511628211ull;
    };
    mix(child, (size_t)cas->nel * nch);
    mix(fbdc, (size_t)nfb);
    mix(cbdc, (size_t)ncb);
  }
  if (!G.d_child || G.key != key) {
    G.key = key;
    FH_TRY(gal_upload(&G.d_child, child, (size_t)cas->nel * nch * sizeof(int)));
    std::vector<unsigned char> cnt((size_t)nch * nc, 0), row((size_t)nch * nc * 8, 0);
    std::vector<double> val((size_t)nch * nc * 8, 0.0), phi(nc), dphi((size_t)nc * 3);
    for (int j = 0; j < nch; j++)
      for (int i = 0; i < nc; i++) {                      // fine node i of child j: C_j[i][k] = phi_k at its reference point in the parent
        double pt[3] = {0, 0, 0};
        fhfe::child_node_ref(cas->geom, j, i, pt);
        fhfe::eval_basis(cas->geom, fhfe::FE_BIQUADRATIC, pt, phi.data(), dphi.data());
        for (int k = 0; k < nc; k++)
          if (std::fabs(phi[k]) > 1e-14) {                // the threshold of ElemType.cpp:439-532
            unsigned char& n = cnt[(size_t)j * nc + k];
            FH_REQUIRE(n < 8, "fh_assembler_galerkin: more than 8 fine nodes of a child depend on one coarse node");
            row[((size_t)j * nc + k) * 8 + n] = (unsigned char)i;
            val[((size_t)j * nc + k) * 8 + n] = phi[k];
            n++;
          }
      }
    {
      std::vector<double> dense((size_t)nch * nc * nc, 0.0);
      for (int j = 0; j < nch; j++)
        for (int k = 0; k < nc; k++)
          for (int q = 0; q < cnt[(size_t)j * nc + k]; q++) dense[((size_t)j * nc + row[((size_t)j * nc + k) * 8 + q]) * nc + k] = val[((size_t)j * nc + k) * 8 + q];
      FH_TRY(gal_upload(&G.d_dense, dense.data(), dense.size() * sizeof(double)));
    }
    FH_TRY(gal_upload(&G.d_cnt, cnt.data(), cnt.size()));
    FH_TRY(gal_upload(&G.d_row, row.data(), row.size()));
    FH_TRY(gal_upload(&G.d_val, val.data(), val.size() * sizeof(double)));
    std::vector<unsigned char> fb(fas->nnode, 0), cb(cas->nnode, 0);
    for (int k = 0; k < nfb; k++) {
      FH_REQUIRE(fbdc[k] >= 0 && fbdc[k] < fas->nnode, "fh_assembler_galerkin: fine Dirichlet node %d out of range", fbdc[k]);
      fb[fbdc[k]] = 1;
    }
    for (int k = 0; k < ncb; k++) {
      FH_REQUIRE(cbdc[k] >= 0 && cbdc[k] < cas->nnode, "fh_assembler_galerkin: coarse Dirichlet node %d out of range", cbdc[k]);
      cb[cbdc[k]] = 1;
    }
    FH_TRY(gal_upload(&G.d_fb, fb.data(), fb.size()));
    FH_TRY(gal_upload(&G.d_cb, cb.data(), cb.size()));
    if (!G.d_res) FH_CHECK_HIP(hipMalloc(&G.d_res, std::max<size_t>(cas->ndof, 1) * sizeof(double)));
    if (nc == 27) {
      if (G.d_fmask) FH_CHECK_HIP(hipFree(G.d_fmask));
      G.d_fmask = nullptr;
      FH_CHECK_HIP(hipMalloc(&G.d_fmask, ((size_t)cas->nel * 9 + 1) * sizeof(unsigned)));
      hipLaunchKernelGGL(k_gal_masks, dim3(fh_div_up(cas->nel * 9, 256)), dim3(256), 0, c->stream, cas->nel, G.d_child, fas->d_elem_dof, fas->nloc, G.d_fb,
                         cas->d_elem_dof, cas->nloc, G.d_cb, G.d_fmask, G.d_fmask + (size_t)cas->nel * 8);
      FH_CHECK_HIP(hipGetLastError());
    }
    // the macro rows of a fused assembly can stand in for the element rows when child j of coarse element E is element j of ONE cluster (what the
    // refinement's numbering gives: MeshRefinement.cpp:240-294)
    G.children_in_order = nch == CL_NE;
    for (int E = 0; E < cas->nel && G.children_in_order; E++)
      for (int j = 0; j < nch; j++)
        if (child[(size_t)E * nch + j] != (child[(size_t)E * nch] / nch) * nch + j || child[(size_t)E * nch] % nch) { G.children_in_order = false; break; }
  }
  // source of the fine element contributions: the macro rows the fused assembly left in the fine matrix and the partial-row buffer (nothing to re-create,
  // the fused path stays the path of the next assembly), or the element-row buffer of the two-pass path
  // Whether the macro rows can still be read back is the fine assembler's to say (fh_assembler_macro_rows: any writer of the fine matrix other than the
  // Dirichlet-row replacement, or its destruction, sends the product back to the element rows, which are re-created from the arguments of the last assembly);
  // the product's own terms are its kernel (Q2 hexahedra, options) and that the children of every coarse element are the elements of one cluster, in order.
  const MacroRows mr = nc == 27 && c->galerkin_mfma && c->galerkin_macro && G.children_in_order ? fh_assembler_macro_rows(fas) : MacroRows();
  const bool from_macro = mr.ok && mr.ncl == cas->nel;
  if (!from_macro) FH_TRY(fh_assembler_need_element_rows(fas));
  const int grid = std::max(1, std::min(fh_div_up(cas->nel, 4), c->num_cu * 2));
  if (from_macro) {
    static bool attr_set_m[64] = {};
    if (!attr_set_m[c->device & 63]) {
      FH_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_galerkin_macro<false>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)gmac_lds_bytes()));
      FH_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_galerkin_macro<true>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)gmac_lds_bytes()));
      attr_set_m[c->device & 63] = true;
    }
    const int gm_grid = std::max(1, std::min(cas->nel, c->num_cu));          // (two workgroups per compute unit would need 128 registers per lane: 101 spilled)
    if (c->asm_debug & 128) {             // dev aid: phase cycles of every wave on stderr (as for the cluster kernel)
      unsigned long long* d_st = nullptr;
      const size_t nst = (size_t)gm_grid * GMAC_NW * 20;
      FH_CHECK_HIP(hipMalloc(&d_st, nst * sizeof(unsigned long long)));
      FH_CHECK_HIP(hipMemsetAsync(d_st, 0, nst * sizeof(unsigned long long), c->stream));
      hipLaunchKernelGGL(k_galerkin_macro<true>, dim3(gm_grid), dim3(GMAC_T), gmac_lds_bytes(), c->stream, cas->nel, G.d_child, mr.nm, mr.sinfo, mr.map,
                         mr.vdst64, mr.gtab, G.d_fmask, G.d_fmask + (size_t)cas->nel * 8, cas->d_slot, cas->d_Kbuf,
                         cas->kstride, G.d_dense, d_st);
      std::vector<unsigned long long> h(nst);
      FH_CHECK_HIP(hipMemcpyAsync(h.data(), d_st, nst * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
      FH_CHECK_HIP(hipStreamSynchronize(c->stream));
      FH_CHECK_HIP(hipFree(d_st));
      static const char* name[10] = {"loop top", "macro matrix into LDS", "barrier", "next cluster's loads issued, look-ups", "K~ fragments gathered, two products (56 MFMA)",
                                     "barrier (all waves done with the macro matrix)", "result into LDS", "barrier", "eight results added, coarse rows stored", "barrier"};
      double sum[10] = {0}, ncl = 0, tot = 0;
      for (size_t w = 0; w < (size_t)gm_grid * GMAC_NW; w++) {
        for (int k = 0; k < 10; k++) sum[k] += (double)h[w * 20 + k];
        ncl += (double)h[w * 20 + 16];
      }
      for (int k = 0; k < 10; k++) tot += sum[k];
      fprintf(stderr, "k_galerkin_macro phase stamps: %.0f shader-clock ticks per cluster and wave\n", tot / std::max(ncl, 1.0));
      for (int k = 0; k < 10; k++) fprintf(stderr, "  %2d %-62s %9.1f  %5.1f %%\n", k, name[k], sum[k] / std::max(ncl, 1.0), 100.0 * sum[k] / std::max(tot, 1.0));
    } else
      hipLaunchKernelGGL(k_galerkin_macro<false>, dim3(gm_grid), dim3(GMAC_T), gmac_lds_bytes(), c->stream, cas->nel, G.d_child, mr.nm, mr.sinfo, mr.map,
                         mr.vdst64, mr.gtab, G.d_fmask, G.d_fmask + (size_t)cas->nel * 8, cas->d_slot, cas->d_Kbuf,
                         cas->kstride, G.d_dense, (unsigned long long*)nullptr);
  } else if (c->galerkin_mfma) {
    const size_t lds = nc == 27 ? galerkin_mfma_lds<27, 8>() : galerkin_mfma_lds<9, 4>();
    static bool attr_set[64] = {};
    if (!attr_set[c->device & 63]) {
      FH_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_galerkin_mfma<27, 8>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)galerkin_mfma_lds<27, 8>()));
      FH_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_galerkin_mfma<9, 4>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)galerkin_mfma_lds<9, 4>()));
      attr_set[c->device & 63] = true;
    }
    const int g1 = std::max(1, std::min(fh_div_up(cas->nel, GAL_NW), c->num_cu));
    if (nc == 27)
      hipLaunchKernelGGL((k_galerkin_mfma<27, 8>), dim3(g1), dim3(GAL_NW * 64), lds, c->stream, cas->nel, G.d_child, fas->d_slot, fas->d_Kbuf, fas->kstride, fas->d_elem_dof,
                         fas->nloc, G.d_fb, cas->d_slot, cas->d_Kbuf, cas->kstride, cas->d_elem_dof, cas->nloc, G.d_cb, G.d_dense);
    else
      hipLaunchKernelGGL((k_galerkin_mfma<9, 4>), dim3(g1), dim3(GAL_NW * 64), lds, c->stream, cas->nel, G.d_child, fas->d_slot, fas->d_Kbuf, fas->kstride, fas->d_elem_dof,
                         fas->nloc, G.d_fb, cas->d_slot, cas->d_Kbuf, cas->kstride, cas->d_elem_dof, cas->nloc, G.d_cb, G.d_dense);
  } else if (nc == 27)
    hipLaunchKernelGGL((k_galerkin_elem<27, 8>), dim3(grid), dim3(256), 0, c->stream, cas->nel, G.d_child, fas->d_slot, fas->d_Kbuf, fas->kstride,
                       fas->d_elem_dof, fas->nloc, G.d_fb, cas->d_slot, cas->d_Kbuf, cas->kstride, cas->d_elem_dof, cas->nloc, G.d_cb, G.d_cnt,
                       G.d_row, G.d_val);
  else
    hipLaunchKernelGGL((k_galerkin_elem<9, 4>), dim3(grid), dim3(256), 0, c->stream, cas->nel, G.d_child, fas->d_slot, fas->d_Kbuf, fas->kstride,
                       fas->d_elem_dof, fas->nloc, G.d_fb, cas->d_slot, cas->d_Kbuf, cas->kstride, cas->d_elem_dof, cas->nloc, G.d_cb, G.d_cnt,
                       G.d_row, G.d_val);
  FH_CHECK_HIP(hipGetLastError());
  FH_CHECK_HIP(hipMemsetAsync(cas->d_Fbuf, 0, std::max<size_t>(cas->nadj, 1) * sizeof(double), c->stream));
  FH_TRY(fh_assembler_row_pass(cas, Ac, G.d_res));
  fh_assembler_rows_replaced(cas);     // the next coarser product reads the coarse element rows; macro rows of an earlier fused assembly into Ac are gone
  fh_mat_values_written(Ac);
  return 0;
  FH_GUARD_END("fh_assembler_galerkin")
}
