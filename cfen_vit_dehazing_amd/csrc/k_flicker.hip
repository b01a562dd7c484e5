// Flicker along the motion (include/cfen_flicker.h states the definition and the contract; tests/flicker_ref.py restates it in numpy).  Scored
// under dehaze_video.py --eval_flicker (flicker.Scorer, ops.flicker_u8).
//
//   k_flicker        : a workgroup (256 threads, 4 waves) owns ONE tile of FK_T x FK_T pixels of one frame.  The vectors of the tile's blocks
//                      (at most 8 x 8; zeros without a field) go to LDS as one dword each.  An item is (row of the tile, group of four linear
//                      pixel indices p = address of the guide frame (mod 4)): such a group starts on a 4-byte boundary whatever the frame's
//                      alignment, so three dword loads fetch it when it lies inside the frame's memory, single bytes otherwise; the target
//                      frame rides on the same groups when its address has the same phase (block-uniform), bytes otherwise.  Per pixel of the
//                      row's span: the block's vector, q = p + v, and where q is inside the frame three bytes of each predecessor; dI and dF
//                      by v_sad_u8 on RGB0 dwords, eF channel by channel.  Seven uint32 sums per thread -> lane butterfly -> the four waves.
//                      One record per workgroup.  The largest entry of a record is 4096 * 3 * 255^2 < 2^32.
//   k_flicker_finish : one workgroup per frame: thread t adds records t, t + 256, ... in uint64, then the butterfly and the four waves.
// Two launches; no global atomics, no counters; all integer, so the order of the additions does not matter.
#include "../../include/cfen_flicker.h"
#include "cfen_image.hpp"

namespace {

constexpr int FK_T = CFEN_FLICKER_TILE;
constexpr int FK_GROUPS = (FK_T + 3 + 3) / 4;                                // four-pixel groups that can touch one row of a tile: 17
constexpr int FK_NCOL = 7;
constexpr int FK_MAX_EDGE = 16384;
constexpr int FK_MAX_BATCH = 65536;

struct FkRecord {
  unsigned v[8];
};
static_assert(sizeof(FkRecord) == CFEN_FLICKER_RECORD_BYTES, "record size");
static_assert(FK_T == 64, "tiles hold whole blocks of 8, 16 and 32, and 4096 * 3 * 255 * 255 < 2^32");

union FkBytes {
  unsigned u[3];
  unsigned char c[12];
};

CFEN_DEV unsigned fk_rgb0(const unsigned char* p) { return (unsigned)p[0] | ((unsigned)p[1] << 8) | ((unsigned)p[2] << 16); }

// the four pixels gp .. gp + 3 of `src`: three dword loads where `dwords` says the group is aligned and inside the frame's memory, else the
// bytes of the pixels inside [L0, L1)
CFEN_DEV void fk_fetch(const unsigned char* src, long long gp, long long L0, long long L1, bool dwords, FkBytes& v) {
  v.u[0] = v.u[1] = v.u[2] = 0u;
  if (dwords) {
    const unsigned* p = reinterpret_cast<const unsigned*>(src + gp * 3);
    v.u[0] = p[0];
    v.u[1] = p[1];
    v.u[2] = p[2];
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (gp + j >= L0 && gp + j < L1) {
        v.c[3 * j] = src[(gp + j) * 3];
        v.c[3 * j + 1] = src[(gp + j) * 3 + 1];
        v.c[3 * j + 2] = src[(gp + j) * 3 + 2];
      }
  }
}

__global__ __launch_bounds__(256) void k_flicker(const unsigned char* guide, const unsigned char* prev_guide, const unsigned char* tgt,
                                                 const unsigned char* prev_tgt, const short* __restrict__ vec, int h, int w, int shift, int bh,
                                                 int bw, int tiles_x, int ntiles, unsigned tol3, FkRecord* __restrict__ rec) {
  __shared__ int sVec[64];                                                     // (dx << 16) | (dy & 0xffff) of the tile's blocks
  __shared__ unsigned red[4][8];
  const int tid = threadIdx.x;
  const int k = blockIdx.x / ntiles, tile = blockIdx.x - k * ntiles;
  const int x0 = (tile % tiles_x) * FK_T, y0 = (tile / tiles_x) * FK_T;
  const long long npix = (long long)h * w, frame = npix * 3;
  const unsigned char* curI = guide + k * frame;
  const unsigned char* prvI = k ? curI - frame : prev_guide;
  const unsigned char* curF = tgt + k * frame;
  const unsigned char* prvF = k ? curF - frame : prev_tgt;
  const int a = (int)(reinterpret_cast<uintptr_t>(curI) & 3);                  // block-uniform: pixel groups p = a (mod 4) are dword aligned
  const bool same_phase = (int)(reinterpret_cast<uintptr_t>(curF) & 3) == a;   // ... in the target frame as well
  const int bpt = FK_T >> shift;                                               // blocks per tile edge: 8, 4, 2
  if (tid < bpt * bpt) {
    const int by = (y0 >> shift) + tid / bpt, bx = (x0 >> shift) + tid % bpt;
    int v = 0;
    if (vec != nullptr && by < bh && bx < bw) v = *reinterpret_cast<const int*>(vec + (((long long)k * bh + by) * bw + bx) * 2);
    sVec[tid] = v;
  }
  __syncthreads();
  const int xe = min(x0 + FK_T, w), rows = min(FK_T, h - y0);
  unsigned acc[FK_NCOL];
#pragma unroll
  for (int c = 0; c < FK_NCOL; ++c) acc[c] = 0u;
  for (int item = tid; item < rows * FK_GROUPS; item += 256) {
    const int ty = item / FK_GROUPS, g = item - ty * FK_GROUPS;
    const int gy = y0 + ty;
    const long long L0 = (long long)gy * w + x0, L1 = (long long)gy * w + xe;  // linear indices of the row's span
    const long long gp = L0 - ((L0 - a) & 3) + 4 * g;                         // first index of the group: gp = a (mod 4), gp <= L0 for g = 0
    if (gp >= L1) continue;
    const bool whole = gp >= 0 && gp + 4 <= npix;                              // wholly inside the frame's memory (it may leave the span)
    FkBytes vi, vf;
    fk_fetch(curI, gp, L0, L1, whole, vi);
    fk_fetch(curF, gp, L0, L1, whole && same_phase, vf);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const long long p = gp + j;
      if (p < L0 || p >= L1) continue;
      const int tx = (int)(p - L0);                                            // column inside the tile
      const int v = sVec[(ty >> shift) * bpt + (tx >> shift)];
      const int qy = gy + (int)(short)(v & 0xffff), qx = x0 + tx + (v >> 16);   // |v| < 2^15 and the frame's edge <= 2^14: no overflow
      if ((unsigned)qy >= (unsigned)h || (unsigned)qx >= (unsigned)w) continue;    // not covered
      const long long q = ((long long)qy * w + qx) * 3;
      const unsigned ci = (unsigned)vi.c[3 * j] | ((unsigned)vi.c[3 * j + 1] << 8) | ((unsigned)vi.c[3 * j + 2] << 16);
      const unsigned cf = (unsigned)vf.c[3 * j] | ((unsigned)vf.c[3 * j + 1] << 8) | ((unsigned)vf.c[3 * j + 2] << 16);
      const unsigned qi = fk_rgb0(prvI + q), qf = fk_rgb0(prvF + q);
      const unsigned dI = __builtin_amdgcn_sad_u8(ci, qi, 0u), dF = __builtin_amdgcn_sad_u8(cf, qf, 0u);
      unsigned eF = 0u;
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const int d = (int)((cf >> (8 * c)) & 255u) - (int)((qf >> (8 * c)) & 255u);
        eF += (unsigned)(d * d);
      }
      const bool m = dI <= tol3;
      acc[0] += 1u;
      acc[1] += m ? 1u : 0u;
      acc[2] += m ? dI : 0u;
      acc[3] += m ? dF : 0u;
      acc[4] += m ? eF : 0u;
      acc[5] += dF;
      acc[6] += dI;
    }
  }
#pragma unroll
  for (int c = 0; c < FK_NCOL; ++c) acc[c] = wave_sum(acc[c]);
  if ((tid & 63) == 0) {
#pragma unroll
    for (int c = 0; c < FK_NCOL; ++c) red[tid >> 6][c] = acc[c];
  }
  __syncthreads();
  if (tid < 8) rec[blockIdx.x].v[tid] = tid < FK_NCOL ? red[0][tid] + red[1][tid] + red[2][tid] + red[3][tid] : 0u;
}

__global__ __launch_bounds__(256) void k_flicker_finish(const FkRecord* __restrict__ rec, int nrec, unsigned long long* __restrict__ sums) {
  __shared__ unsigned long long red[4][8];
  const int tid = threadIdx.x;
  const FkRecord* p = rec + (size_t)blockIdx.x * nrec;
  unsigned long long s[FK_NCOL];
#pragma unroll
  for (int c = 0; c < FK_NCOL; ++c) s[c] = 0ull;
  for (int i = tid; i < nrec; i += 256) {
    const uint2* r = reinterpret_cast<const uint2*>(&p[i]);                    // scratch is 8-byte aligned: four 8-byte loads
    const uint2 r0 = r[0], r1 = r[1], r2 = r[2], r3 = r[3];
    s[0] += r0.x, s[1] += r0.y, s[2] += r1.x, s[3] += r1.y, s[4] += r2.x, s[5] += r2.y, s[6] += r3.x;
  }
#pragma unroll
  for (int c = 0; c < FK_NCOL; ++c) s[c] = wave_sum(s[c]);
  if ((tid & 63) == 0) {
#pragma unroll
    for (int c = 0; c < FK_NCOL; ++c) red[tid >> 6][c] = s[c];
  }
  __syncthreads();
  if (tid < 8) sums[(size_t)blockIdx.x * 8 + tid] = tid < FK_NCOL ? red[0][tid] + red[1][tid] + red[2][tid] + red[3][tid] : 0ull;
}

bool fk_dims_ok(int B, int h, int w) { return B >= 1 && B <= FK_MAX_BATCH && h >= 1 && w >= 1 && h <= FK_MAX_EDGE && w <= FK_MAX_EDGE; }

int fk_tiles_x(int w) { return (w + FK_T - 1) / FK_T; }
int fk_tiles_y(int h) { return (h + FK_T - 1) / FK_T; }                     // tiles per frame <= 2^16

bool fk_overlap(const void* p, long long np, const void* q, long long nq) {
  const uintptr_t a = reinterpret_cast<uintptr_t>(p), b = reinterpret_cast<uintptr_t>(q);
  return p && q && a < b + (uintptr_t)nq && b < a + (uintptr_t)np;
}

}  // namespace

extern "C" size_t cfen_flicker_bytes(int B, int h, int w) {
  if (!fk_dims_ok(B, h, w)) return 0;
  const long long blocks = (long long)B * fk_tiles_x(w) * fk_tiles_y(h);
  return blocks <= 0x7fffffffLL ? (size_t)blocks * sizeof(FkRecord) : 0;
}

extern "C" int cfen_flicker_u8(const unsigned char* guide, const unsigned char* prev_guide, const unsigned char* tgt, const unsigned char* prev_tgt,
                               const short* vec, int B, int h, int w, int block, int tol, void* scratch, unsigned long long* sums, void* stream) {
  CFEN_CHECK_ARG(guide && prev_guide && tgt && prev_tgt && scratch && sums,
                 "flicker_u8: null pointer (guide, prev_guide, tgt, prev_tgt, scratch and sums are all required)");
  CFEN_CHECK_ARG(B >= 1 && B <= FK_MAX_BATCH, "flicker_u8: B = %d outside 1 .. %d", B, FK_MAX_BATCH);
  CFEN_CHECK_ARG(h >= 1 && w >= 1 && h <= FK_MAX_EDGE && w <= FK_MAX_EDGE, "flicker_u8: sizes h = %d, w = %d outside 1 .. %d", h, w, FK_MAX_EDGE);
  CFEN_CHECK_ARG(block == 8 || block == 16 || block == 32, "flicker_u8: block = %d is none of 8, 16, 32", block);
  CFEN_CHECK_ARG(tol >= 0 && tol <= 255, "flicker_u8: tol = %d outside 0 .. 255", tol);
  CFEN_CHECK_ARG(cfen_aligned(vec, 4), "flicker_u8: vec must be 4-byte aligned");
  CFEN_CHECK_ARG(cfen_aligned(scratch, 8) && cfen_aligned(sums, 8), "flicker_u8: scratch and sums must be 8-byte aligned (64-bit words)");
  const int tiles_x = fk_tiles_x(w), ntiles = tiles_x * fk_tiles_y(h);
  const int bh = (h + block - 1) / block, bw = (w + block - 1) / block;
  const long long px = (long long)h * w, blocks = (long long)B * ntiles;
  CFEN_CHECK_ARG(blocks <= 0x7fffffffLL, "flicker_u8: B = %d frames of %d x %d are too large for one launch", B, h, w);
  const void* const in[5] = {guide, prev_guide, tgt, prev_tgt, vec};
  const long long in_bytes[5] = {B * px * 3, px * 3, B * px * 3, px * 3, (long long)B * bh * bw * 4};
  const long long scratch_bytes = blocks * (long long)sizeof(FkRecord), sums_bytes = (long long)B * 64;
  bool apart = !fk_overlap(scratch, scratch_bytes, sums, sums_bytes);
  for (int i = 0; i < 5; ++i)
    apart = apart && !fk_overlap(scratch, scratch_bytes, in[i], in_bytes[i]) && !fk_overlap(sums, sums_bytes, in[i], in_bytes[i]);
  CFEN_CHECK_ARG(apart, "flicker_u8: scratch and sums must not overlap each other or any input");
  hipStream_t s = (hipStream_t)stream;
  const int shift = block == 8 ? 3 : block == 16 ? 4 : 5;
  CFEN_LAUNCH(k_flicker, dim3((unsigned)blocks), dim3(256), 0, s, guide, prev_guide, tgt, prev_tgt, vec, h, w, shift, bh, bw, tiles_x, ntiles,
              (unsigned)(3 * tol), (FkRecord*)scratch);
  CFEN_CHECK_LAUNCH("flicker_u8");
  CFEN_LAUNCH(k_flicker_finish, dim3((unsigned)B), dim3(256), 0, s, (const FkRecord*)scratch, ntiles, sums);
  CFEN_CHECK_LAUNCH("flicker_u8 (finish)");
  return CFEN_OK;
}
