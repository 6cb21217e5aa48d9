// PATA-EC novelty kernels for POET environment reproduction.
//
// An environment is characterised by how all K agents score on it: the
// scores of a column are clipped and turned into integer rank codes
// (pata_ec_codes), and the novelty of a candidate environment is the mean
// Euclidean distance between its code vector and those of its k nearest
// neighbours among the reference (active + archived) environments
// (pata_ec_knn).  Everything is integer arithmetic up to the final square
// roots, so codes and squared distances are exact and the float tail has
// a derived bound (fiber_amd/es/novelty_oracle.py).
//
// This file is a translation unit of its own: it shares no device code
// with the rollout kernels and must not move their register allocation.

#include <hip/hip_runtime.h>
#include <stdint.h>

#define PATA_K_MAX 512   // agents; keeps D2 <= K * 4 (K-1)^2 < 2^31
#define PATA_KNN_MAX 64  // neighbours kept per query

// ---------------------------------------------------------------------------
// pata_ec_codes: scores[K][M] fp32 -> codes[M][Kpad] int16
//
// One block per tile of CODES_TC columns.  The tile is read through LDS
// with adjacent threads on adjacent columns (the stride between agents is
// M floats), ranked by the O(K^2) count out of LDS, staged as int16 rows
// and written out as one contiguous run of 16-byte stores: the rows of a
// tile are adjacent in codes[M][Kpad].
// ---------------------------------------------------------------------------
#define CODES_TC 16
#define CODES_THREADS 256
#define CODES_IB 4  // agents ranked per pass over the column

extern "C" __global__ void __launch_bounds__(CODES_THREADS)
pata_ec_codes(const float* __restrict__ scores,  // [K][M]
              int K, int M, int Kpad, float lo, float hi,
              int16_t* __restrict__ codes)  // [M][Kpad]
{
  __shared__ float col[PATA_K_MAX][CODES_TC];                  // 32 KiB
  __shared__ __attribute__((aligned(16))) int16_t
      out[CODES_TC * PATA_K_MAX];                              // 16 KiB
  const int tid = threadIdx.x;
  const int m0 = blockIdx.x * CODES_TC;
  const int ncols = min(CODES_TC, M - m0);

  for (int idx = tid; idx < K * CODES_TC; idx += CODES_THREADS) {
    const int j = idx / CODES_TC, c = idx % CODES_TC;
    float x = lo;  // columns past M: never written out
    if (c < ncols) {
      const float s = scores[(size_t)j * M + m0 + c];
      // NaN fails; +-inf clip to hi / lo
      x = (s != s) ? lo : fminf(fmaxf(s, lo), hi);
    }
    col[j][c] = x;
  }
  // the pad entries of every row are 0, so they add nothing to a distance
  const int npad = Kpad - K;
  for (int idx = tid; idx < npad * CODES_TC; idx += CODES_THREADS)
    out[(idx / npad) * Kpad + K + idx % npad] = 0;
  __syncthreads();

  // thread -> (column c, agents slot, slot + 16, ...), CODES_IB at a time
  const int c = tid % CODES_TC;
  const int slot = tid / CODES_TC;
  constexpr int SLOTS = CODES_THREADS / CODES_TC;
  for (int i0 = slot; i0 < K; i0 += SLOTS * CODES_IB) {
    float ci[CODES_IB];
    int lt[CODES_IB], eq[CODES_IB];
#pragma unroll
    for (int u = 0; u < CODES_IB; ++u) {
      const int i = i0 + u * SLOTS;
      ci[u] = col[i < K ? i : i0][c];
      lt[u] = 0;
      eq[u] = 0;
    }
    for (int j = 0; j < K; ++j) {
      const float cj = col[j][c];
#pragma unroll
      for (int u = 0; u < CODES_IB; ++u) {
        lt[u] += cj < ci[u];
        eq[u] += cj == ci[u];  // -0.0 == +0.0: a tie
      }
    }
#pragma unroll
    for (int u = 0; u < CODES_IB; ++u) {
      const int i = i0 + u * SLOTS;
      // twice the mid-rank, in [0, 2 (K-1)]
      if (i < K) out[c * Kpad + i] = (int16_t)(2 * lt[u] + eq[u] - 1);
    }
  }
  __syncthreads();

  // Kpad % 8 == 0: whole 16-byte vectors, the tile is one contiguous run
  const int nvec = ncols * (Kpad / 8);
  const uint4* __restrict__ src = reinterpret_cast<const uint4*>(out);
  uint4* __restrict__ dst =
      reinterpret_cast<uint4*>(codes + (size_t)m0 * Kpad);
  for (int v = tid; v < nvec; v += CODES_THREADS) dst[v] = src[v];
}

// ---------------------------------------------------------------------------
// pata_ec_knn: for each query row q in [n_ref, n_ref + Q) of codes, the
// k smallest D2(q, r) = sum_i (code[q][i] - code[r][i])^2 over the
// reference rows r in [0, n_ref), ascending, and their novelty.
//
// One block serves KNN_QT queries per pass over the references.  The
// references stream through LDS in tiles of KNN_REFS rows x 64 codes,
// loaded with 16-byte loads (8 codes) that cover whole 128-byte row
// segments; a thread owns KNN_RPT rows of the tile and accumulates one
// exact int32 D2 per (row, query) with a packed 16-bit subtract and the
// signed 16-bit dot-product-accumulate (|diff| <= 1022 fits int16).  The
// LDS row stride is 144 B (36 dwords), which spreads the 16 lanes of a
// ds_read_b128 group over all 64 banks.
//
// After a tile of references each thread holds KNN_RPT candidates per
// query.  best[q] is the ascending list of the k smallest so far; rounds
// of a block-wide min pull the candidates below its last entry in one at
// a time (all queries per round), so a reference tile costs as many
// rounds as it improves the list, k at the most.  Duplicated distances
// are separate candidates: the (distance, slot) key makes each min
// unique.
// ---------------------------------------------------------------------------
#define KNN_QT 4
#define KNN_RPT 2
#define KNN_THREADS 256
#define KNN_REFS (KNN_THREADS * KNN_RPT)
#define KNN_ROW4 9  // uint4 per LDS row: 8 of codes + 1 of padding

typedef short pata_short2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ int sq_acc2(uint32_t a, uint32_t b, int acc) {
  const pata_short2 d = __builtin_bit_cast(pata_short2, a) -
                        __builtin_bit_cast(pata_short2, b);
  return __builtin_amdgcn_sdot2(d, d, acc, false);
}

__device__ __forceinline__ int sq_acc8(const uint4& a, const uint4& b,
                                       int acc) {
  acc = sq_acc2(a.x, b.x, acc);
  acc = sq_acc2(a.y, b.y, acc);
  acc = sq_acc2(a.z, b.z, acc);
  return sq_acc2(a.w, b.w, acc);
}

static_assert(KNN_QT == KNN_THREADS / 64,
              "wave w inserts into the list of query w");

extern "C" __global__ void __launch_bounds__(KNN_THREADS)
pata_ec_knn(const int16_t* __restrict__ codes,  // [n_ref + Q][Kpad]
            int Kpad, int K, int n_ref, int Q, int k,  // k <= min(64, n_ref)
            int* __restrict__ knn_d2,       // [Q][k]
            float* __restrict__ novelty)    // [Q]
{
  __shared__ uint4 ref_t[KNN_REFS * KNN_ROW4];          // 72 KiB
  __shared__ uint4 qrow[KNN_QT][PATA_K_MAX / 8];        // 4 KiB
  __shared__ int best[KNN_QT][PATA_KNN_MAX];
  __shared__ unsigned long long wmin[KNN_THREADS / 64][KNN_QT];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int q0 = blockIdx.x * KNN_QT;
  const int nch = Kpad / 8;  // 16-byte chunks per row, <= 64
  const uint4* __restrict__ codes4 = reinterpret_cast<const uint4*>(codes);
  const unsigned long long NONE = ~0ull;

  // the block's query rows; a slot past Q repeats the last query and is
  // not written out
  for (int idx = tid; idx < KNN_QT * nch; idx += KNN_THREADS) {
    const int qi = idx / nch, ch = idx % nch;
    const int q = min(q0 + qi, Q - 1);
    qrow[qi][ch] = codes4[(size_t)(n_ref + q) * nch + ch];
  }
  for (int idx = tid; idx < KNN_QT * PATA_KNN_MAX; idx += KNN_THREADS)
    best[idx / PATA_KNN_MAX][idx % PATA_KNN_MAX] = INT_MAX;

  for (int r0 = 0; r0 < n_ref; r0 += KNN_REFS) {
    int acc[KNN_RPT][KNN_QT];
#pragma unroll
    for (int rp = 0; rp < KNN_RPT; ++rp)
#pragma unroll
      for (int qi = 0; qi < KNN_QT; ++qi) acc[rp][qi] = 0;

    for (int c0 = 0; c0 < nch; c0 += 8) {
      const int tc = min(8, nch - c0);
      __syncthreads();  // the previous tile has been consumed
      for (int idx = tid; idx < KNN_REFS * 8; idx += KNN_THREADS) {
        const int row = idx >> 3, ch = idx & 7;
        const int r = r0 + row;
        uint4 v = make_uint4(0u, 0u, 0u, 0u);
        if (r < n_ref && ch < tc) v = codes4[(size_t)r * nch + c0 + ch];
        ref_t[row * KNN_ROW4 + ch] = v;
      }
      __syncthreads();
      for (int ch = 0; ch < tc; ++ch) {
        uint4 rv[KNN_RPT];
#pragma unroll
        for (int rp = 0; rp < KNN_RPT; ++rp)
          rv[rp] = ref_t[(tid + rp * KNN_THREADS) * KNN_ROW4 + ch];
#pragma unroll
        for (int qi = 0; qi < KNN_QT; ++qi) {
          const uint4 qv = qrow[qi][c0 + ch];  // same address: broadcast
#pragma unroll
          for (int rp = 0; rp < KNN_RPT; ++rp)
            acc[rp][qi] = sq_acc8(rv[rp], qv, acc[rp][qi]);
        }
      }
    }

    // rows past n_ref are no candidates
#pragma unroll
    for (int rp = 0; rp < KNN_RPT; ++rp)
      if (r0 + tid + rp * KNN_THREADS >= n_ref)
#pragma unroll
        for (int qi = 0; qi < KNN_QT; ++qi) acc[rp][qi] = INT_MAX;

    // ---- merge the tile's candidates into best[] -----------------------
    for (;;) {
#pragma unroll
      for (int qi = 0; qi < KNN_QT; ++qi) {
        const int thr = best[qi][k - 1];
        unsigned long long key = NONE;
#pragma unroll
        for (int rp = 0; rp < KNN_RPT; ++rp)
          if (acc[rp][qi] < thr) {
            const unsigned long long cand =
                ((unsigned long long)(unsigned)acc[rp][qi] << 16) |
                (unsigned)(rp * KNN_THREADS + tid);
            key = cand < key ? cand : key;
          }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
          const unsigned long long o = __shfl_xor(key, off, 64);
          key = o < key ? o : key;
        }
        if (lane == 0) wmin[wave][qi] = key;
      }
      __syncthreads();
      bool any = false;
#pragma unroll
      for (int qi = 0; qi < KNN_QT; ++qi) {
        unsigned long long m = wmin[0][qi];
#pragma unroll
        for (int w = 1; w < KNN_THREADS / 64; ++w)
          m = wmin[w][qi] < m ? wmin[w][qi] : m;
        if (m == NONE) continue;
        any = true;
        const int val = (int)(m >> 16);
        const int slot = (int)(m & 0xFFFFu);
#pragma unroll
        for (int rp = 0; rp < KNN_RPT; ++rp)
          if (slot == rp * KNN_THREADS + tid) acc[rp][qi] = INT_MAX;
        if (wave == qi) {
          // sorted insert, lane j owns best[qi][j]; the entry pushed past
          // the end drops out
          const int a = best[qi][lane];
          const int b = __shfl_up(a, 1, 64);
          const bool left_le = (lane == 0) || (b <= val);
          best[qi][lane] = (a <= val) ? a : (left_le ? val : b);
        }
      }
      __syncthreads();
      if (!any) break;  // block-uniform: every thread read the same wmin
    }
  }

  // ---- outputs: one thread per query, a fixed ascending-order sum ------
  if (tid < KNN_QT && q0 + tid < Q) {
    const int q = q0 + tid;
    float sum = 0.f;
    for (int j = 0; j < k; ++j) {
      const int d2 = best[tid][j];
      knn_d2[(size_t)q * k + j] = d2;
      sum += sqrtf((float)d2);
    }
    novelty[q] = sum / (float)(k * 2 * (K - 1));
  }
}
