// The body of k_wino_conv / k_wino_conv_strided (wino.hip, which documents it): included into both kernels with TC, RAG, SPLIT, STR and
// the argument `a` in scope.  No include guard: it is meant to be included more than once.
  constexpr int DEAD = STR == 1 ? 3 : (STR == 2 ? 0 : -1);         // the xi-column whose planes are identically zero
  constexpr int TR = WN_TILES / TC;
  constexpr int RH = 2 * TR + 2, RW = 2 * TC + 2;
  constexpr int NPIX = RH * RW, NRI = (NPIX + 31) / 32;      // raw patch: pixels, 1 KiB DMA pieces (32 pixels x 32 B)
  constexpr int RAWBUF = NRI * 256;                             // floats
  constexpr int NR_IT = (NRI + 7) / 8;                          // DMA pieces per wave
  constexpr int BUF = 2 * 16 * WN_PLANE;                        // floats of one (V, U) buffer pair
  static_assert((2 * BUF + 2 * RAWBUF) * 4 <= 163840, "LDS budget");
  __shared__ __attribute__((aligned(16))) float lds[2 * BUF + 2 * RAWBUF];
  float* rawbase = lds + 2 * BUF;
  // chunk ch lives in buffer (ch + 1) & 1: chunk 0 of the NEXT group can then be fetched into the upper buffer while the epilogue of
  // the current group uses the lower 74 KB as its exchange / transposition space
#define WN_BUFOF(CH) (lds + (((CH) + 1) & 1) * BUF)

  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int li = lane & 31, half = lane >> 5;
  const int mb = wave & 1, nb = (wave >> 1) & 1, xh = wave >> 2;
  const int KT = a.K / WN_KB;
  const int tiles_w = RAG ? ((a.W + 1) / 2 + TC - 1) / TC : (a.W / 2) / TC;
  const int tiles_h = RAG ? ((a.H + 1) / 2 + TR - 1) / TR : (a.H / 2) / TR;
  const int nsplit = SPLIT ? a.splits : 1;
  const int ngroups = a.N * tiles_h * tiles_w * KT * nsplit;
  const int nchunks = a.C / WN_CK / nsplit;                           // chunks per workgroup (the launcher makes the split exact)

  // transform role of this thread: tile, channel quad, column b of the 4x4 domain
  // Round 6: column b is WAVE-UNIFORM (it was the lane's low bits): which raw columns combine is then an address, the sign a scalar
  // register, and row i of T = d B is two packed fused multiply-adds d[i][jA] + sgn d[i][jB] (a product with +-1 is exact, the sum is
  // rounded once: the values of round 3's sg0 d[j0] + sg1 d[j1]).  Next to v_mfma_f32_32x32x2_f32 a VALU instruction is NOT free (it costs
  // the SIMD ~3.3 cycles of matrix time, a packed one 5.3: tools/exp/mfma_overlap.hip); the masks of the rows outside the image and the
  // sign multiplications were 60 of the transform's 94 instructions per wave and chunk.
  const int tb = wave & 3, tc4 = lane & 1, ttile = (wave >> 2) * 32 + (lane >> 1);
  const int ttr = ttile / TC, ttc = ttile % TC;
  const int j0 = tb == 0 ? 0 : (tb == 2 ? 2 : 1), j1 = tb == 2 ? 1 : (tb == 3 ? 3 : 2);      // b = 0: d0 - d2, 1: d1 + d2, 2: d2 - d1, 3: d1 - d3
  const float sgn_s = tb == 1 ? 1.f : -1.f;
  const f32x2 sgn = {sgn_s, sgn_s};
  const int t_wr = tb * WN_PLANE + ttile * 8 + ((tc4 ^ ((ttile >> 3) & 1)) * 4);
  const int t_rd = ((2 * ttr) * RW + 2 * ttc) * 8 + tc4 * 4;        // raw(row 0, col 0) of this tile's window
  // DMA pieces of this wave (round 6: the pieces of a wave are neighbours in LDS and share ONE M0 write -- the immediate offset of
  // global_load_lds moves the LDS address and the global address together (tools/exp/pk_probe.hip); an M0 write per piece, with the
  // v_readfirstlane in front of it, was half of the DMA's cost):
  //   raw: pieces 2 wave, 2 wave + 1 of the patch (pixels 32 piece + lane / 2, channel quad lane & 1; rows outside the image read row
  //        0 / H-1 and are zeroed by the transform), the second one 1 KiB behind the first -- its scalar base is 1 KiB lower;
  //   U:   planes 2 wave, 2 wave + 1 of the chunk's 32 KiB block (wn_u_index), a linear copy: every piece has the per-lane offset 16 lane;
  //        the planes lie 2112 bytes apart in LDS and 2048 in memory, so the second plane's base is 64 bytes lower.
  constexpr int NRAW_W = (NRI + 1) / 2;                          // waves that have raw pieces
  const unsigned lane16 = 16u * (unsigned)lane;
  const int arow = mb * 32 + li, brow = nb * 32 + li;
  const int a_off = arow * 8 + ((half ^ ((arow >> 3) & 1)) * 4);
  const int b_off = 16 * WN_PLANE + brow * 8 + ((half ^ ((brow >> 3) & 1)) * 4);

  // (tile group, channel block) of the group in hand: persistent workgroups -- the grid is capped at the number of CUs (one
  // 512-thread workgroup fits a CU) and every workgroup walks its share of the groups, fetching the first operands of its NEXT
  // group while the epilogue of the current one runs
  int n, k0, gh, gw;
  int cb = 0;                                                           // first chunk of this workgroup's channel range (SPLIT)
  float* ysp = a.y;                                                     // where this group's result goes (SPLIT: its range's partial plane)
  const float* xn;
  int rowmask[4];                                                     // zero rows above / below the image ...
  bool edge;                                                          // ... which only the first / last row of tile groups has (uniform)
  unsigned raw_g[NR_IT];
#define WN_SETUP(G, LN)                                                                                                   \
  {                                                                                                                       \
    int t_ = wn_xcd_swizzle((G), ngroups);                                                                                \
    if (SPLIT) { cb = (t_ % nsplit) * nchunks; t_ /= nsplit; }       /* the ranges of one (tiles, channels) block are neighbours */ \
    const int kt_ = t_ % KT; t_ /= KT;                                                                                    \
    gw = t_ % tiles_w; t_ /= tiles_w;                                                                                     \
    gh = t_ % tiles_h;                                                                                                    \
    n = t_ / tiles_h;                                                                                                     \
    k0 = kt_ * WN_KB;                                                                                                     \
    const int h_base_ = gh * TR * 2 - 1, w_base_ = gw * TC * 2 - 1;          /* image position of raw(0,0) */             \
    xn = a.x + (size_t)n * a.H * a.W * a.C;                                                                               \
    _Pragma("unroll") for (int i = 0; i < 4; ++i) {                                                                       \
      const int h_ = h_base_ + 2 * ttr + i;                                                                               \
      rowmask[i] = (h_ >= 0 && h_ < a.H) ? -1 : 0;                                                                        \
    }                                                                                                                     \
    edge = __builtin_amdgcn_readfirstlane((int)(h_base_ < 0 || h_base_ + RH > a.H)) != 0;                                                                           \
    _Pragma("unroll") for (int it = 0; it < NR_IT; ++it) {                                                                \
      const int p_ = min(min(2 * wave + it, NRI - 1) * 32 + ((LN) >> 1), NPIX - 1);        /* recomputed: registers are scarce */ \
      int h_ = h_base_ + p_ / RW;                                                                                         \
      h_ = h_ < 0 ? 0 : (h_ >= a.H ? a.H - 1 : h_);                                                                       \
      int w_ = w_base_ + p_ % RW;                                                                                         \
      if (RAG) { w_ %= a.W; w_ = w_ < 0 ? w_ + a.W : w_; }       /* surplus columns of an overhanging group lie beyond 2W */ \
      else w_ = w_ < 0 ? w_ + a.W : (w_ >= a.W ? w_ - a.W : w_);                                                           \
      raw_g[it] = 4u * (unsigned)((h_ * a.W + w_) * a.C + ((LN) & 1) * 4);          /* bytes */                             \
    }                                                                                                                     \
  }

  // LDS DMA: 64 lanes x 16 bytes per piece from (wave-uniform base) + (per-lane byte offset) to the LDS address M0 + immediate + 16 lane.
  // Issued from inline assembly (see CH_GLDS in convh_common.h): while a global_load_lds BUILTIN is outstanding the compiler turns every
  // LDS wait into s_waitcnt lgkmcnt(0); hidden from it, the fragment / transform reads are waited for individually.  Every barrier that
  // hands DMA-written data over is preceded by an explicit s_waitcnt vmcnt(0) -- __syncthreads() alone does NOT wait for these loads.
  const unsigned lds_base = (unsigned)(__SIZE_TYPE__)((__attribute__((address_space(3))) char*)lds);
  const int m0_raw = __builtin_amdgcn_readfirstlane((int)(lds_base + 4u * (unsigned)(2 * BUF + min(2 * wave, NRI - 1) * 256)));      // raw buffer 0
  const int m0_u = __builtin_amdgcn_readfirstlane((int)(lds_base + 4u * (unsigned)(16 * WN_PLANE + 2 * wave * WN_PLANE)));            // (V, U) buffer 0
#define WN_RAW_ALL(CH)                                                                                                    \
  {                                                                                                                       \
    const float* rp_ = xn + ((CH) + cb) * WN_CK;                                                                          \
    const int m_ = m0_raw + ((CH) & 1) * (RAWBUF * 4);                                                                    \
    if (2 * wave + 1 < NRI)                                                                                               \
      asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %3\n\tglobal_load_lds_dwordx4 %2, %4 offset:1024"     \
                   :: "s"(m_), "v"(raw_g[0]), "v"(raw_g[NR_IT - 1]), "s"(rp_), "s"(rp_ - 256) : "memory");                  \
    else if (2 * wave < NRI)                                                                                              \
      asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2" :: "s"(m_), "v"(raw_g[0]), "s"(rp_) : "memory");  \
  }
#define WN_U_ALL(CH, BUFP)                                                                                                \
  {                                                                                                                       \
    const float* up_ = a.u + (((size_t)((CH) + cb) * KT + (k0 >> 6)) * 16 + 2 * wave) * 512;                               \
    const int m_ = m0_u + (int)((BUFP) - lds) * 4;                                                                        \
    if (DEAD == 3 && (wave & 1))                                      /* plane 2 wave + 1 is zero: never read */           \
      asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2\n\tglobal_load_lds_dwordx4 %1, %2 offset:1024" \
                   :: "s"(m_), "v"(lane16), "s"(up_) : "memory");                                                         \
    else if (DEAD == 0 && !(wave & 1))                                /* plane 2 wave is zero */                           \
      asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2 offset:2112\n\tglobal_load_lds_dwordx4 %1, %2 offset:3136" \
                   :: "s"(m_), "v"(lane16), "s"(up_ - 16) : "memory");                                                    \
    else                                                                                                                  \
    asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2\n\tglobal_load_lds_dwordx4 %1, %2 offset:1024\n\t" \
                 "global_load_lds_dwordx4 %1, %3 offset:2112\n\tglobal_load_lds_dwordx4 %1, %3 offset:3136"                \
                 :: "s"(m_), "v"(lane16), "s"(up_), "s"(up_ - 16) : "memory");                                            \
  }
  // row I of T = d B for this thread's column: two 16-byte reads of the raw patch (issued ahead of their use: a read and its use in
  // the same slice stalls the wave for an LDS round trip while its partner on the SIMD is in the same phase), masked for rows
  // outside the image
#define WN_TROW_LD(I, RB)                                                                                                 \
  {                                                                                                                       \
    dd[(I) & 1][0] = *reinterpret_cast<const i32x4*>((RB) + t_rd + ((I) * RW + j0) * 8);                                  \
    dd[(I) & 1][1] = *reinterpret_cast<const i32x4*>((RB) + t_rd + ((I) * RW + j1) * 8);                                  \
  }
#define WN_TROW_FIN(I)                                                                                                    \
  {                                                                                                                       \
    if (edge) { asm volatile("" ::: "memory"); dd[(I) & 1][0] &= rowmask[I]; dd[(I) & 1][1] &= rowmask[I]; }     /* (a real branch) */ \
    const f32x4 da_ = __builtin_bit_cast(f32x4, dd[(I) & 1][0]), db_ = __builtin_bit_cast(f32x4, dd[(I) & 1][1]);         \
    asm volatile("v_pk_fma_f32 %0, %1, %2, %3" : "=v"(tt[I][0]) : "v"(__builtin_shufflevector(db_, db_, 0, 1)), "s"(sgn), "v"(__builtin_shufflevector(da_, da_, 0, 1))); \
    asm volatile("v_pk_fma_f32 %0, %1, %2, %3" : "=v"(tt[I][1]) : "v"(__builtin_shufflevector(db_, db_, 2, 3)), "s"(sgn), "v"(__builtin_shufflevector(da_, da_, 2, 3))); \
  }
#define WN_TROW(I, RB) WN_TROW_LD(I, RB) WN_TROW_FIN(I)
  // x + y / x - y of four channels as two packed instructions (inline assembly: the compiler scalarises the plain vector expressions)
#define WN_PK_ADD(X, Y) ({ f32x2 l_, h_;                                                                                    \
    asm volatile("v_pk_add_f32 %0, %1, %2" : "=v"(l_) : "v"((X)[0]), "v"((Y)[0]));                                        \
    asm volatile("v_pk_add_f32 %0, %1, %2" : "=v"(h_) : "v"((X)[1]), "v"((Y)[1]));                                        \
    __builtin_shufflevector(l_, h_, 0, 1, 2, 3); })
#define WN_PK_SUB(X, Y) ({ f32x2 l_, h_;                                                                                    \
    asm volatile("v_pk_add_f32 %0, %1, %2 neg_lo:[0,1] neg_hi:[0,1]" : "=v"(l_) : "v"((X)[0]), "v"((Y)[0]));              \
    asm volatile("v_pk_add_f32 %0, %1, %2 neg_lo:[0,1] neg_hi:[0,1]" : "=v"(h_) : "v"((X)[1]), "v"((Y)[1]));              \
    __builtin_shufflevector(l_, h_, 0, 1, 2, 3); })
  // V(0) of the group in hand from its raw(0): the one transform that is not hidden behind MFMAs
#define WN_V0()                                                                                                           \
  {                                                                                                                       \
    f32x2 tt[4][2];                                                                                                       \
    i32x4 dd[2][2];                                                                                                       \
    const float* rb_ = rawbase;                                                                                           \
    float* vb_ = WN_BUFOF(0) + t_wr;                                                                                      \
    WN_TROW(0, rb_) WN_TROW(1, rb_) WN_TROW(2, rb_) WN_TROW(3, rb_)                                                       \
    *reinterpret_cast<f32x4*>(vb_ + 0 * 4 * WN_PLANE) = WN_PK_SUB(tt[0], tt[2]);                                                    \
    *reinterpret_cast<f32x4*>(vb_ + 1 * 4 * WN_PLANE) = WN_PK_ADD(tt[1], tt[2]);                                                    \
    *reinterpret_cast<f32x4*>(vb_ + 2 * 4 * WN_PLANE) = WN_PK_SUB(tt[2], tt[1]);                                                    \
    *reinterpret_cast<f32x4*>(vb_ + 3 * 4 * WN_PLANE) = WN_PK_SUB(tt[1], tt[3]);                                                    \
  }
#define WN_LOAD_FRAGS_FROM(XL, BP)                                                                                        \
  {                                                                                                                       \
    av[(XL) & 1] = *reinterpret_cast<const f32x4*>((BP) + (xh * 8 + (XL)) * WN_PLANE + a_off);                            \
    bv[(XL) & 1] = *reinterpret_cast<const f32x4*>((BP) + (xh * 8 + (XL)) * WN_PLANE + b_off);                            \
  }
#define WN_LOAD_FRAGS(XL) WN_LOAD_FRAGS_FROM(XL, cur)
#define WN_M(XL, J, ...)                                                                                                  \
  {                                                                                                                       \
    acc[XL] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[(XL) & 1][J], bv[(XL) & 1][J], acc[XL], 0, 0, 0);                   \
    __VA_ARGS__                                                                                                           \
    __builtin_amdgcn_sched_barrier(0);                                                                                    \
  }
  // the first MFMA of a plane in the first chunk of a group: C = 0 (an inline constant: the 128 accumulator registers are never zeroed)
#define WN_MZ(XL, J, ...)                                                                                                 \
  {                                                                                                                       \
    acc[XL] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[(XL) & 1][J], bv[(XL) & 1][J], wn_zero16, 0, 0, 0);                 \
    __VA_ARGS__                                                                                                           \
    __builtin_amdgcn_sched_barrier(0);                                                                                    \
  }
  // STR: the six live planes of a wave alternate between the two fragment registers by their position, not by their index
#define WN_LOAD_FRAGS_B(XL, B, BP)                                                                                        \
  {                                                                                                                       \
    av[B] = *reinterpret_cast<const f32x4*>((BP) + (xh * 8 + (XL)) * WN_PLANE + a_off);                                   \
    bv[B] = *reinterpret_cast<const f32x4*>((BP) + (xh * 8 + (XL)) * WN_PLANE + b_off);                                   \
  }
#define WN_MB(XL, B, J, ...)                                                                                              \
  {                                                                                                                       \
    acc[XL] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[B][J], bv[B][J], acc[XL], 0, 0, 0);                                 \
    __VA_ARGS__                                                                                                           \
    __builtin_amdgcn_sched_barrier(0);                                                                                    \
  }
#define WN_MZB(XL, B, J, ...)                                                                                             \
  {                                                                                                                       \
    acc[XL] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[B][J], bv[B][J], wn_zero16, 0, 0, 0);                               \
    __VA_ARGS__                                                                                                           \
    __builtin_amdgcn_sched_barrier(0);                                                                                    \
  }

  const f32x16 wn_zero16 = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  int grp = blockIdx.x;                              // the launcher guarantees gridDim.x <= ngroups
  WN_SETUP(grp, lane)
  // prologue of the first group: raw(0), raw(1), U(0) -> LDS; V(0) from raw(0)
  WN_RAW_ALL(0)
  WN_RAW_ALL(min(1, nchunks - 1))
  WN_U_ALL(0, WN_BUFOF(0))
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  WN_V0()
  for (;;) {
    __syncthreads();
    WN_T(0)
    f32x4 av[2], bv[2];                              // (declared per group: nothing of them is carried from one group to the next)
    f32x2 tt[4][2];
    i32x4 dd[2][2];
    f32x16 acc[8];                                   // (never zeroed: the first MFMA of a plane in the group's first chunk takes C = 0)
    {
      float* cur = WN_BUFOF(0);
      if (DEAD == 0) WN_LOAD_FRAGS_B(1, 0, cur)
      else WN_LOAD_FRAGS(0)
    }
    // Pipeline (one barrier per chunk).  LDS holds two (V, U) buffers and two raw-patch buffers.  While the waves multiply chunk c:
    //   * the LDS DMA (global_load_lds, no registers) brings U of chunk c+1 into the other (V, U) buffer and the raw input patch of
    //     chunk c+2 -- (2TR+2) x (2TC+2) pixels x 8 channels, wrap-around columns by addressing -- into raw[c & 1]; both have the
    //     whole chunk to land;
    //   * every thread turns the raw patch of chunk c+1 (raw[(c+1) & 1], landed during chunk c-1) into its column b of
    //     V = B^T d B for its (tile, channel quad): 8 x 16-byte LDS reads, a few adds, 4 x 16-byte LDS writes.
    // All of that is sliced into small pieces placed behind individual MFMAs: in-order issue means a wave's next MFMA on the same
    // accumulator cannot issue for 64 cycles anyway, and a piece runs in that shadow.  The fences keep hipcc from sinking every
    // piece to its first use.  The barrier of a chunk sits in front of its LAST plane: every wave holds that plane's fragments in
    // registers by then, so its four MFMAs run behind the barrier and cover the fetch of the next chunk's first fragments.
    // (Fetching the raw pieces straight into registers -- 8 scattered 16-byte loads per thread and chunk, each 32-byte pixel slice
    // requested by ~4 threads -- measured 15 % slower: the vector-memory path, not the matrix pipe, became the limit.)
#define WN_CHUNK_BODY(MF)                                                                                                 \
    {                                                                                                                     \
      float* cur = WN_BUFOF(ch);                                                                                          \
      float* nxt = WN_BUFOF(ch + 1);                                                                                      \
      const float* rb = rawbase + ((ch + 1) & 1) * RAWBUF;                                                                \
      float* vb = nxt + t_wr;                                                                                             \
      MF(0, 0, WN_IF_FR(WN_LOAD_FRAGS(1))) WN_M(0, 1, WN_IF_U(WN_U_ALL(ch + 1, nxt)))                                     \
      WN_M(0, 2, )                                                                                                        \
      /* raw(ch+2) overwrites raw(ch), which every wave finished reading before the last barrier */                      \
      WN_M(0, 3, WN_IF_RAW(if (ch + 2 < nchunks) WN_RAW_ALL(ch + 2)))                                                     \
      /* LDS reads in the first two slices of a plane, arithmetic in the last two: whatever a plane's first MFMA waits for is two slices old */ \
      MF(1, 0, WN_IF_FR(WN_LOAD_FRAGS(2))) WN_M(1, 1, WN_IF_T(WN_TROW_LD(0, rb) WN_TROW_LD(1, rb))) WN_M(1, 2, ) WN_M(1, 3, WN_IF_T(WN_TROW_FIN(0) WN_TROW_FIN(1))) \
      MF(2, 0, WN_IF_FR(WN_LOAD_FRAGS(3))) WN_M(2, 1, WN_IF_T(WN_TROW_LD(2, rb) WN_TROW_LD(3, rb))) WN_M(2, 2, ) WN_M(2, 3, WN_IF_T(WN_TROW_FIN(2) WN_TROW_FIN(3))) \
      MF(3, 0, WN_IF_FR(WN_LOAD_FRAGS(4)) WN_IF_T(*reinterpret_cast<f32x4*>(vb + 0 * 4 * WN_PLANE) = WN_PK_SUB(tt[0], tt[2]);))   \
      WN_M(3, 1, WN_IF_T(*reinterpret_cast<f32x4*>(vb + 1 * 4 * WN_PLANE) = WN_PK_ADD(tt[1], tt[2]);)) WN_M(3, 2, ) WN_M(3, 3, ) \
      MF(4, 0, WN_IF_FR(WN_LOAD_FRAGS(5)) WN_IF_T(*reinterpret_cast<f32x4*>(vb + 2 * 4 * WN_PLANE) = WN_PK_SUB(tt[2], tt[1]);))   \
      WN_M(4, 1, WN_IF_T(*reinterpret_cast<f32x4*>(vb + 3 * 4 * WN_PLANE) = WN_PK_SUB(tt[1], tt[3]);)) WN_M(4, 2, ) WN_M(4, 3, ) \
      MF(5, 0, WN_IF_FR(WN_LOAD_FRAGS(6))) WN_M(5, 1, ) WN_M(5, 2, ) WN_M(5, 3, )                                         \
      MF(6, 0, WN_IF_FR(WN_LOAD_FRAGS(7))) WN_M(6, 1, ) WN_M(6, 2, ) WN_M(6, 3, )                                         \
      asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");                                                         \
      WN_IF_BAR(__builtin_amdgcn_s_barrier();)                                                                            \
      __builtin_amdgcn_sched_barrier(0);                                                                                  \
      MF(7, 0, WN_IF_FR(WN_LOAD_FRAGS_FROM(0, nxt))) WN_M(7, 1, ) WN_M(7, 2, ) WN_M(7, 3, )                               \
    }
#define WN_TAIL_BODY(MF)                                                                                                  \
    {                                                                                                                     \
      float* cur = WN_BUFOF(nchunks - 1);                                                                                 \
      MF(0, 0, WN_LOAD_FRAGS(1)) WN_M(0, 1, ) WN_M(0, 2, ) WN_M(0, 3, )                                                   \
      MF(1, 0, WN_LOAD_FRAGS(2)) WN_M(1, 1, ) WN_M(1, 2, ) WN_M(1, 3, )                                                   \
      MF(2, 0, WN_LOAD_FRAGS(3)) WN_M(2, 1, ) WN_M(2, 2, ) WN_M(2, 3, )                                                   \
      MF(3, 0, WN_LOAD_FRAGS(4)) WN_M(3, 1, ) WN_M(3, 2, ) WN_M(3, 3, )                                                   \
      MF(4, 0, WN_LOAD_FRAGS(5)) WN_M(4, 1, ) WN_M(4, 2, ) WN_M(4, 3, )                                                   \
      MF(5, 0, WN_LOAD_FRAGS(6)) WN_M(5, 1, ) WN_M(5, 2, ) WN_M(5, 3, )                                                   \
      MF(6, 0, WN_LOAD_FRAGS(7)) WN_M(6, 1, ) WN_M(6, 2, ) WN_M(6, 3, )                                                   \
      MF(7, 0, ) WN_M(7, 1, ) WN_M(7, 2, ) WN_M(7, 3, )                                                                   \
    }
    // STR: the same pipeline over the six live planes of a wave.  The side work of a dead plane's slots moves to free slots of the live
    // ones (no new work is added); the barrier sits in front of the last live plane.  Every wave still transforms its column, the
    // dead one included: values defined under a branch in this loop cost the register allocator 25 registers and spills.
#define WN_TX(...) { __VA_ARGS__ }
#define WN_VST(I, EXPR) WN_TX(*reinterpret_cast<f32x4*>(vb + (I) * 4 * WN_PLANE) = EXPR;)
    // forward, xi-column 3 dead: planes 0 1 2 4 5 6
#define WN_CHUNK_BODY_F(MF)                                                                                               \
    {                                                                                                                     \
      float* cur = WN_BUFOF(ch);                                                                                          \
      float* nxt = WN_BUFOF(ch + 1);                                                                                      \
      const float* rb = rawbase + ((ch + 1) & 1) * RAWBUF;                                                                \
      float* vb = nxt + t_wr;                                                                                             \
      MF(0, 0, 0, WN_LOAD_FRAGS_B(1, 1, cur)) WN_MB(0, 0, 1, WN_U_ALL(ch + 1, nxt)) WN_MB(0, 0, 2, )                      \
      WN_MB(0, 0, 3, if (ch + 2 < nchunks) WN_RAW_ALL(ch + 2))                                                            \
      MF(1, 1, 0, WN_LOAD_FRAGS_B(2, 0, cur)) WN_MB(1, 1, 1, WN_TX(WN_TROW_LD(0, rb) WN_TROW_LD(1, rb))) WN_MB(1, 1, 2, ) \
      WN_MB(1, 1, 3, WN_TX(WN_TROW_FIN(0) WN_TROW_FIN(1)))                                                                \
      MF(2, 0, 0, WN_LOAD_FRAGS_B(4, 1, cur)) WN_MB(2, 0, 1, WN_TX(WN_TROW_LD(2, rb) WN_TROW_LD(3, rb))) WN_MB(2, 0, 2, ) \
      WN_MB(2, 0, 3, WN_TX(WN_TROW_FIN(2) WN_TROW_FIN(3)))                                                                \
      MF(4, 1, 0, WN_LOAD_FRAGS_B(5, 0, cur) WN_VST(0, WN_PK_SUB(tt[0], tt[2])))                                          \
      WN_MB(4, 1, 1, WN_VST(1, WN_PK_ADD(tt[1], tt[2]))) WN_MB(4, 1, 2, ) WN_MB(4, 1, 3, )                                \
      MF(5, 0, 0, WN_LOAD_FRAGS_B(6, 1, cur) WN_VST(2, WN_PK_SUB(tt[2], tt[1])))                                          \
      WN_MB(5, 0, 1, WN_VST(3, WN_PK_SUB(tt[1], tt[3]))) WN_MB(5, 0, 2, ) WN_MB(5, 0, 3, )                                \
      asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");                                                         \
      __builtin_amdgcn_s_barrier();                                                                                       \
      __builtin_amdgcn_sched_barrier(0);                                                                                  \
      MF(6, 1, 0, WN_LOAD_FRAGS_B(0, 0, nxt)) WN_MB(6, 1, 1, ) WN_MB(6, 1, 2, ) WN_MB(6, 1, 3, )                          \
    }
#define WN_TAIL_BODY_F(MF)                                                                                                \
    {                                                                                                                     \
      float* cur = WN_BUFOF(nchunks - 1);                                                                                 \
      MF(0, 0, 0, WN_LOAD_FRAGS_B(1, 1, cur)) WN_MB(0, 0, 1, ) WN_MB(0, 0, 2, ) WN_MB(0, 0, 3, )                          \
      MF(1, 1, 0, WN_LOAD_FRAGS_B(2, 0, cur)) WN_MB(1, 1, 1, ) WN_MB(1, 1, 2, ) WN_MB(1, 1, 3, )                          \
      MF(2, 0, 0, WN_LOAD_FRAGS_B(4, 1, cur)) WN_MB(2, 0, 1, ) WN_MB(2, 0, 2, ) WN_MB(2, 0, 3, )                          \
      MF(4, 1, 0, WN_LOAD_FRAGS_B(5, 0, cur)) WN_MB(4, 1, 1, ) WN_MB(4, 1, 2, ) WN_MB(4, 1, 3, )                          \
      MF(5, 0, 0, WN_LOAD_FRAGS_B(6, 1, cur)) WN_MB(5, 0, 1, ) WN_MB(5, 0, 2, ) WN_MB(5, 0, 3, )                          \
      MF(6, 1, 0, ) WN_MB(6, 1, 1, ) WN_MB(6, 1, 2, ) WN_MB(6, 1, 3, )                                                    \
    }
    // input gradient, xi-column 0 dead: planes 1 2 3 5 6 7
#define WN_CHUNK_BODY_B(MF)                                                                                               \
    {                                                                                                                     \
      float* cur = WN_BUFOF(ch);                                                                                          \
      float* nxt = WN_BUFOF(ch + 1);                                                                                      \
      const float* rb = rawbase + ((ch + 1) & 1) * RAWBUF;                                                                \
      float* vb = nxt + t_wr;                                                                                             \
      MF(1, 0, 0, WN_LOAD_FRAGS_B(2, 1, cur) WN_U_ALL(ch + 1, nxt))                                                       \
      WN_MB(1, 0, 1, WN_TX(WN_TROW_LD(0, rb) WN_TROW_LD(1, rb)))                                                          \
      WN_MB(1, 0, 2, if (ch + 2 < nchunks) WN_RAW_ALL(ch + 2)) WN_MB(1, 0, 3, WN_TX(WN_TROW_FIN(0) WN_TROW_FIN(1)))       \
      MF(2, 1, 0, WN_LOAD_FRAGS_B(3, 0, cur)) WN_MB(2, 1, 1, WN_TX(WN_TROW_LD(2, rb) WN_TROW_LD(3, rb))) WN_MB(2, 1, 2, ) \
      WN_MB(2, 1, 3, WN_TX(WN_TROW_FIN(2) WN_TROW_FIN(3)))                                                                \
      MF(3, 0, 0, WN_LOAD_FRAGS_B(5, 1, cur) WN_VST(0, WN_PK_SUB(tt[0], tt[2])))                                          \
      WN_MB(3, 0, 1, WN_VST(1, WN_PK_ADD(tt[1], tt[2]))) WN_MB(3, 0, 2, ) WN_MB(3, 0, 3, )                                \
      MF(5, 1, 0, WN_LOAD_FRAGS_B(6, 0, cur) WN_VST(2, WN_PK_SUB(tt[2], tt[1])))                                          \
      WN_MB(5, 1, 1, WN_VST(3, WN_PK_SUB(tt[1], tt[3]))) WN_MB(5, 1, 2, ) WN_MB(5, 1, 3, )                                \
      MF(6, 0, 0, WN_LOAD_FRAGS_B(7, 1, cur)) WN_MB(6, 0, 1, ) WN_MB(6, 0, 2, ) WN_MB(6, 0, 3, )                          \
      asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");                                                         \
      __builtin_amdgcn_s_barrier();                                                                                       \
      __builtin_amdgcn_sched_barrier(0);                                                                                  \
      MF(7, 1, 0, WN_LOAD_FRAGS_B(1, 0, nxt)) WN_MB(7, 1, 1, ) WN_MB(7, 1, 2, ) WN_MB(7, 1, 3, )                          \
    }
#define WN_TAIL_BODY_B(MF)                                                                                                \
    {                                                                                                                     \
      float* cur = WN_BUFOF(nchunks - 1);                                                                                 \
      MF(1, 0, 0, WN_LOAD_FRAGS_B(2, 1, cur)) WN_MB(1, 0, 1, ) WN_MB(1, 0, 2, ) WN_MB(1, 0, 3, )                          \
      MF(2, 1, 0, WN_LOAD_FRAGS_B(3, 0, cur)) WN_MB(2, 1, 1, ) WN_MB(2, 1, 2, ) WN_MB(2, 1, 3, )                          \
      MF(3, 0, 0, WN_LOAD_FRAGS_B(5, 1, cur)) WN_MB(3, 0, 1, ) WN_MB(3, 0, 2, ) WN_MB(3, 0, 3, )                          \
      MF(5, 1, 0, WN_LOAD_FRAGS_B(6, 0, cur)) WN_MB(5, 1, 1, ) WN_MB(5, 1, 2, ) WN_MB(5, 1, 3, )                          \
      MF(6, 0, 0, WN_LOAD_FRAGS_B(7, 1, cur)) WN_MB(6, 0, 1, ) WN_MB(6, 0, 2, ) WN_MB(6, 0, 3, )                          \
      MF(7, 1, 0, ) WN_MB(7, 1, 1, ) WN_MB(7, 1, 2, ) WN_MB(7, 1, 3, )                                                    \
    }
    if (DEAD == 3) {
      if (nchunks > 1) {
        { const int ch = 0; WN_CHUNK_BODY_F(WN_MZB) }
        for (int ch = 1; ch + 1 < nchunks; ++ch) WN_CHUNK_BODY_F(WN_MB)
        WN_TAIL_BODY_F(WN_MB)
      } else WN_TAIL_BODY_F(WN_MZB)
    } else if (DEAD == 0) {
      if (nchunks > 1) {
        { const int ch = 0; WN_CHUNK_BODY_B(WN_MZB) }
        for (int ch = 1; ch + 1 < nchunks; ++ch) WN_CHUNK_BODY_B(WN_MB)
        WN_TAIL_BODY_B(WN_MB)
      } else WN_TAIL_BODY_B(WN_MZB)
    } else
    if (nchunks > 1) {
      { const int ch = 0; WN_CHUNK_BODY(WN_MZ) }
      for (int ch = 1; ch + 1 < nchunks; ++ch) WN_CHUNK_BODY(WN_M)
      WN_TAIL_BODY(WN_M)
    } else WN_TAIL_BODY(WN_MZ)
#undef WN_CHUNK_BODY
#undef WN_TAIL_BODY
#undef WN_CHUNK_BODY_F
#undef WN_TAIL_BODY_F
#undef WN_CHUNK_BODY_B
#undef WN_TAIL_BODY_B
#undef WN_TX
#undef WN_VST
    __syncthreads();                                 // every wave is done with the staging buffers
    WN_T(1)

    // Everything the epilogue derives from the lane id is derived from an opaque copy of it: hoisted out of the persistent loop those
    // values would have to live -- or be spilled -- across the chunk loop, where every register is taken
    int lane_e = lane;
    asm volatile("" : "+v"(lane_e));
    const int li_e = lane_e & 31, half_e = lane_e >> 5;
    // Output offsets of this lane's eight epilogue items (item i = lane + 64 it: row = i >> 3 = tile_in_block * 2 + q, channel
    // quad i & 7), taken before the group variables move on
    // (round 6: item it = tile 4 (8 mb + it) + (lane >> 4) of the block, pixel column q = (lane >> 3) & 1: the tile's row / column of the group
    // and the image row are wave-uniform -- scalar arithmetic -- and the lane contributes one offset that is the same for all eight items;
    // the generic per-item div / mod cost ~140 vector instructions per group, and outside the chunk loop the vector ALU is the bottleneck)
    unsigned ooff[8];                                // (element offsets fit 31 bits: checked by the entry point)
    {
      const int lcol = (lane_e >> 4) * 2 + ((lane_e >> 3) & 1);          // pixel column of the lane relative to its item's first tile
      const unsigned lane_off = (unsigned)(lcol * a.K + (lane_e & 7) * 4);
#pragma unroll
      for (int it = 0; it < 8; ++it) {
        const int ut = 4 * (mb * 8 + it), tr = ut / TC, tc = ut % TC;   // (uniform)
        const int oh = (gh * TR + tr) * 2 + xh, ow0 = (gw * TC + tc) * 2;
        ooff[it] = (unsigned)(((n * a.H + oh) * a.W + ow0) * a.K + k0 + nb * 32) + lane_off;
        if (RAG && (oh >= a.H || ow0 + lcol >= a.W)) ooff[it] = 0xffffffffu;       // a surplus pixel (offsets are below 2^31)
      }
    }
    // STR = 2: where the compact grid operand [N][H][W][K/2] has this lane's items; only the even-pixel channel blocks (k0 < K/2) add it
    unsigned goff[8];
    bool grid_block = true;
    if (STR == 2) {
      const int kh = a.K >> 1;
      const int lcol = (lane_e >> 4) * 2 + ((lane_e >> 3) & 1);
      grid_block = k0 < kh;                                              // (uniform: K/2 is a multiple of the 64-channel block)
#pragma unroll
      for (int it = 0; it < 8; ++it) {
        const int ut = 4 * (mb * 8 + it), tr = ut / TC, tc = ut % TC;
        const int oh = (gh * TR + tr) * 2 + xh, ow0 = (gw * TC + tc) * 2;
        goff[it] = grid_block ? (unsigned)(((n * a.H + oh) * a.W + ow0 + lcol) * kh + k0 + nb * 32 + (lane_e & 7) * 4) : 0u;
      }
    }
    const unsigned (&aoff)[8] = STR == 2 ? goff : ooff;                 // offsets of the `add` operand
    if (SPLIT) ysp = a.y + (size_t)(cb / nchunks) * ((size_t)a.N * a.H * a.W * a.K);
    // The first operands of the NEXT group are requested now: raw(0), raw(1) into the raw buffers, U(0) into the upper (V, U) buffer --
    // none of them is touched by the epilogue below, whose duration covers their latency.
    const int nextg = grp + gridDim.x;
    const bool more = nextg < ngroups;
    if (more) {
      WN_SETUP(nextg, lane_e)
      WN_RAW_ALL(0)
      WN_RAW_ALL(min(1, nchunks - 1))
      WN_U_ALL(0, WN_BUFOF(0))
    }

    // The contribution to the partner's row goes to LDS as soon as it exists (exchange region per (block, direction): 2 x 16 x 64
    // floats in the lower staging buffer, which is free): the accumulators, both halves of the result and the loop-carried
    // addressing state of the persistent loop do not fit the register file together.
    f32x16 keep[2];
    float* xch = lds;
    const int blk = wave & 3;                          // (mb, nb) block; partner = wave ^ 4
    {
      float* dst = xch + ((blk * 2 + xh) * 32) * 64 + lane_e;
#pragma unroll
      for (int q = 0; q < 2; ++q) {
        f32x16 p0, p1;                                  // P[2xh][q], P[2xh+1][q]
        if (DEAD == 0) {                                // (planes 0 and 4 never ran: exact zeros)
          if (q == 0) { p0 = acc[1] + acc[2]; p1 = acc[5] + acc[6]; }
          else        { p0 = wn_sub16(wn_sub16(acc[1], acc[2]), acc[3]); p1 = wn_sub16(wn_sub16(acc[5], acc[6]), acc[7]); }
        } else if (DEAD == 3) {                         // (planes 3 and 7)
          if (q == 0) { p0 = acc[0] + acc[1] + acc[2]; p1 = acc[4] + acc[5] + acc[6]; }
          else        { p0 = wn_sub16(acc[1], acc[2]); p1 = wn_sub16(acc[5], acc[6]); }
        } else
        if (q == 0) { p0 = acc[0] + acc[1] + acc[2]; p1 = acc[4] + acc[5] + acc[6]; }
        else        { p0 = wn_sub16(wn_sub16(acc[1], acc[2]), acc[3]); p1 = wn_sub16(wn_sub16(acc[5], acc[6]), acc[7]); }
        f32x16 snd;
        if (xh == 0) { keep[q] = p0 + p1; snd = p1; }              // rows 0,1: Y0 += P0 + P1, Y1 += P1
        else         { keep[q] = wn_nsub16(p0, p1); snd = p0; }    // rows 2,3: Y0 += P2,      Y1 += -P2 - P3
#pragma unroll
        for (int r = 0; r < 16; ++r) dst[(q * 16 + r) * 64] = snd[r];
        __builtin_amdgcn_sched_barrier(0);
      }
    }
    const bool f_add = (a.epi & WN_EPI_ADD) && (STR != 2 || grid_block), f_act = a.epi & WN_EPI_ACT, f_dact = a.epi & WN_EPI_DACT;
    __syncthreads();
    {
      const float* src = xch + ((blk * 2 + (xh ^ 1)) * 32) * 64 + lane_e;
#pragma unroll
      for (int q = 0; q < 2; ++q)
#pragma unroll
        for (int r = 0; r < 16; ++r) keep[q][r] += src[(q * 16 + r) * 64];
    }
    __syncthreads();
    WN_T(2)
    // keep[q][r] = output pixel (row 2*tr + xh, col 2*tc + q) of tile (r & 3) + 8 * (r >> 2) + 4 * half of this block, channel li.
    // Transposed through LDS per wave (32 tiles x 2 pixels x 32 channels; all of it inside the lower staging buffer) so that a lane
    // owns four consecutive channels: float4 epilogue arithmetic and 16-byte stores of 128-byte channel rows.
    constexpr int ES = 32;
    static_assert(8 * 64 * ES <= BUF, "the transposition space must stay inside the lower (V, U) buffer");
    float* ep = lds + wave * (64 * ES);
#pragma unroll
    for (int q = 0; q < 2; ++q)
#pragma unroll
      for (int r = 0; r < 16; ++r) ep[(((r & 3) + 8 * (r >> 2) + 4 * half_e) * 2 + q) * ES + li_e] = keep[q][r];
    // Epilogue operand of this lane's eight output rows (the saved activation of an input-gradient pass, else the shortcut),
    // requested in one batch as soon as the registers of the result are free: its latency runs under the wait for the next group's
    // operands instead of in front of every store (the compiler cannot batch the loads itself: y may alias them as far as it
    // knows).  A pass with both operands fetches the shortcut in the store loop.
    f32x4 opv[8];
    {
      // (unconditional: without an operand every lane re-reads the first 16 bytes of the weights -- cheaper than what the register
      // allocator does with conditionally defined values in this loop)
      const bool has_op = f_dact || f_add;
      const float* op = f_dact ? a.dsrc : (f_add ? a.add : a.u);
#pragma unroll
      for (int it = 0; it < 8; ++it) opv[it] = *reinterpret_cast<const f32x4*>(op + ((has_op && (!RAG || ooff[it] != 0xffffffffu)) ? (STR == 2 && !f_dact ? goff[it] : ooff[it]) : 0u));
    }
    if (more) {
      // the next group's operands have landed (the stores of this group are issued AFTER this wait, so they are never waited
      // for); V(0) of the next group goes into the upper buffer, which the epilogue does not touch
      asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();
      __builtin_amdgcn_sched_barrier(0);
      WN_V0()
    }
    WN_T(3)
    const bool tanh_act = a.act == 1;
    if (tanh_act || !(f_act || f_dact)) {
      const float* epl = ep + (lane_e >> 3) * ES + (lane_e & 7) * 4;
      if (f_dact) { if (f_add) wn_store_items<true, false, true, RAG>(epl, opv, ooff, aoff, ysp, a.add); else wn_store_items<false, false, true, RAG>(epl, opv, ooff, aoff, ysp, a.add); }
      else if (f_act) { if (f_add) wn_store_items<true, true, false, RAG>(epl, opv, ooff, aoff, ysp, a.add); else wn_store_items<false, true, false, RAG>(epl, opv, ooff, aoff, ysp, a.add); }
      else { if (f_add) wn_store_items<true, false, false, RAG>(epl, opv, ooff, aoff, ysp, a.add); else wn_store_items<false, false, false, RAG>(epl, opv, ooff, aoff, ysp, a.add); }
    } else
#pragma unroll
    for (int it = 0; it < 8; ++it) {
      const int i = lane_e + it * 64, row = i >> 3, c4 = i & 7;
      if (RAG && ooff[it] == 0xffffffffu) continue;
      f32x4 v = *reinterpret_cast<const f32x4*>(ep + row * ES + c4 * 4);
      if (f_add) v += f_dact ? *reinterpret_cast<const f32x4*>(a.add + aoff[it]) : opv[it];
      if (f_act) {
        if (tanh_act) { v[0] = dl_tanh(v[0]); v[1] = dl_tanh(v[1]); v[2] = dl_tanh(v[2]); v[3] = dl_tanh(v[3]); }
        else { v[0] = wn_act(v[0], a.act); v[1] = wn_act(v[1], a.act); v[2] = wn_act(v[2], a.act); v[3] = wn_act(v[3], a.act); }
      }
      if (f_dact) {
        const f32x4 sv = opv[it];
        if (tanh_act) v *= 1.f - sv * sv;
        else { v[0] *= wn_dact(sv[0], a.act); v[1] *= wn_dact(sv[1], a.act); v[2] *= wn_dact(sv[2], a.act); v[3] *= wn_dact(sv[3], a.act); }
      }
      *reinterpret_cast<f32x4*>(ysp + ooff[it]) = v;
    }
    WN_T(4)
    if (!more) break;
    grp = nextg;
  }
#undef WN_BUFOF
#undef WN_SETUP
#undef WN_RAW_ALL
#undef WN_U_ALL
#undef WN_TROW
#undef WN_PK_ADD
#undef WN_PK_SUB
#undef WN_TROW_LD
#undef WN_TROW_FIN
#undef WN_V0
#undef WN_LOAD_FRAGS
#undef WN_LOAD_FRAGS_FROM
#undef WN_M
#undef WN_MZ
#undef WN_LOAD_FRAGS_B
#undef WN_MB
#undef WN_MZB
