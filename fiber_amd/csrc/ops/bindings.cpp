// Python bindings for the ES CDNA4 kernels (fiber_amd._ops).
//
// Deliberately torch-header-free: tensors cross as raw device pointers +
// the current HIP stream (integers from the Python wrapper,
// fiber_amd/ops/__init__.py), which keeps the extension a plain hipcc
// build and the launch path thin.

#include <hip/hip_bf16.h>
#include <hip/hip_runtime.h>
#include <pybind11/pybind11.h>
#include <rocprim/rocprim.hpp>

#include <stdexcept>
#include <string>

#include "me_grid.h"

namespace py = pybind11;

#define NPARAMS_HOST 4610
#define ENVS_HOST 64
#define OBS_HOST 4

extern "C" __global__ void es_rollout_mlp(
    const float*, float, uint32_t, uint32_t, int, int, const float*,
    const float*, const float*, const float*, float*, float*, float*);
extern "C" __global__ void es_eval_matrix(const float*, const float*,
                                          const float*, const float*,
                                          const float*, uint32_t, uint32_t,
                                          int, int, float*, float*);
extern "C" __global__ void obs_stat_reduce(const float*, int, float*);
extern "C" __global__ void es_grad(const float*, int, int, int, uint32_t,
                                   uint32_t, int, float*);
extern "C" __global__ void es_grad_reduce(const float*, int, int, float*);
extern "C" __global__ void centered_rank(const float*, int, float*);
extern "C" __global__ void rank_pack_keys(const float*, int, unsigned*,
                                          unsigned*);
extern "C" __global__ void rank_scatter(const unsigned*, int, float*);
extern "C" __global__ void mlp_policy_forward(const float*, const float*,
                                              int, float*);
extern "C" __global__ void mfma_gemm64_probe(const float*, const float*,
                                             float*);
extern "C" __global__ void logits_reduce_probe(const float*, const float*,
                                               float*, float*);
// per-pair batched kernels (es_pairs_kernels.hip)
extern "C" __global__ void es_rollout_mlp_pairs(
    const float*, float, const uint32_t*, uint32_t, int, int, const float*,
    const float*, const float*, const float*, float*, float*, float*);
extern "C" __global__ void obs_stat_reduce_pairs(const float*, int, float*);
extern "C" __global__ void centered_rank_pairs(const float*, int, float*);
extern "C" __global__ void es_grad_pairs(const float*, int, int,
                                         const uint32_t*, uint32_t, int,
                                         float*);
extern "C" __global__ void es_grad_reduce_pairs(const float*, int, int,
                                                float*);
// novelty-search kernels (ns_kernels.hip)
extern "C" __global__ void es_rollout_mlp_bc(
    const float*, float, uint32_t, uint32_t, int, int, const float*,
    const float*, const float*, const float*, float*, float*, float*, float*,
    float*);
extern "C" __global__ void es_eval_bc(const float*, const float*,
                                      const float*, const float*,
                                      const float*, uint32_t, uint32_t, int,
                                      int, float*, float*, float*, float*);
extern "C" __global__ void bc_knn_novelty(const float*, int, const float*,
                                          int, int, float*, float*);
// separable-NES kernels (snes_kernels.hip)
extern "C" __global__ void es_rollout_mlp_sigma(
    const float*, const float*, uint32_t, uint32_t, int, int, const float*,
    const float*, const float*, const float*, float*, float*, float*);
extern "C" __global__ void es_grad_sigma(const float*, const float*, int,
                                         int, int, uint32_t, uint32_t, int,
                                         float*);
// Deep GA kernels (ga_kernels.hip)
extern "C" __global__ void ga_parents(uint32_t, uint32_t, int, int, uint32_t,
                                      int*, int*);
extern "C" __global__ void ga_rollout_mlp(
    const float*, const int*, const int*, float, uint32_t, uint32_t, int,
    const float*, const float*, const float*, const float*, float*, float*,
    float*);
extern "C" __global__ void ga_truncate(const float*, int, int, int*);
extern "C" __global__ void ga_survivors(const float*, const int*, const int*,
                                        const int*, float, uint32_t, uint32_t,
                                        float*);
extern "C" __global__ void ga_decode(const float*, const int*, int, float,
                                     uint32_t, float*);
// safe-mutation kernels (sm_kernels.hip)
extern "C" __global__ void sm_steps(const float*, const float*, float, float,
                                    int, float*, float*);
extern "C" __global__ void ga_rollout_mlp_sm(
    const float*, const float*, const int*, const int*, uint32_t, uint32_t,
    int, const float*, const float*, const float*, const float*, float*,
    float*, float*);
extern "C" __global__ void ga_survivors_sm(const float*, const float*,
                                           const int*, const int*, const int*,
                                           uint32_t, uint32_t, float*);
// MAP-Elites kernels (me_kernels.hip)
extern "C" __global__ void me_parents(uint32_t, uint32_t, int, const int*,
                                      const int*, int, int*, int*);
extern "C" __global__ void ga_rollout_mlp_bc(
    const float*, const int*, const int*, float, uint32_t, uint32_t, int,
    const float*, const float*, const float*, const float*, float*, float*,
    float*, float*, float*);
extern "C" __global__ void me_assign(const float*, const float*, int, MeGrid,
                                     int*, unsigned long long*);
extern "C" __global__ void me_commit(const float*, const float*, int, int,
                                     const unsigned long long*, float*,
                                     float*, int*, int*, int*);
extern "C" __global__ void me_compact(const int*, int, int*, int*);
// conv policy pipeline (conv_kernels.hip)
// PATA-EC novelty kernels (poet_kernels.hip)
extern "C" __global__ void pata_ec_codes(const float*, int, int, int, float,
                                         float, int16_t*);
extern "C" __global__ void pata_ec_knn(const int16_t*, int, int, int, int,
                                       int, int*, float*);

extern "C" __global__ void es_perturb(const float*, int, int, float,
                                      uint32_t, const uint32_t*, int,
                                      __hip_bfloat16*, unsigned char*,
                                      unsigned char*);
extern "C" __global__ void conv_env_init(uint32_t, const uint32_t*, int,
                                         float*, float*);
extern "C" __global__ void conv_noisegen(uint32_t, const uint32_t*,
                                         uint32_t, unsigned char*);
extern "C" __global__ void conv_layer1(const __hip_bfloat16*,
                                       const unsigned char*, const float*,
                                       const __hip_bfloat16*,
                                       const unsigned char*, int,
                                       __hip_bfloat16*);
extern "C" __global__ void conv_layer2(const __hip_bfloat16*,
                                       const __hip_bfloat16*, int,
                                       unsigned char*);
extern "C" __global__ void conv_fc(const __hip_bfloat16*,
                                   const unsigned char*,
                                   const unsigned char*, int,
                                   __hip_bfloat16*);
extern "C" __global__ void conv_head_env(const __hip_bfloat16*,
                                         const __hip_bfloat16*, int,
                                         const float*, const float*, float*,
                                         float*);

static void check(hipError_t err, const char* what) {
  if (err != hipSuccess) {
    throw std::runtime_error(std::string(what) + ": " +
                             hipGetErrorString(err));
  }
}

static void launch_rollout(uintptr_t theta, double sigma, uint32_t seed,
                           uint32_t iter, int horizon, int member_offset,
                           int pop_shard, uintptr_t obs_mu, uintptr_t obs_nu,
                           uintptr_t env_A, uintptr_t env_B,
                           uintptr_t fitness, uintptr_t obs_stat_part,
                           uintptr_t obs_stat, uintptr_t stream) {
  if (pop_shard <= 0) return;
  hipLaunchKernelGGL(es_rollout_mlp, dim3(pop_shard), dim3(256), 0,
                     (hipStream_t)stream, (const float*)theta, (float)sigma,
                     seed, iter, horizon, member_offset,
                     (const float*)obs_mu, (const float*)obs_nu,
                     (const float*)env_A, (const float*)env_B,
                     (float*)fitness, (float*)obs_stat_part,
                     (float*)obs_stat);
  check(hipGetLastError(), "es_rollout_mlp launch");
  // obs_stat_part is [pop_shard][2*OBS]; one block per stat column
  hipLaunchKernelGGL(obs_stat_reduce, dim3(2 * OBS_HOST), dim3(256), 0,
                     (hipStream_t)stream, (const float*)obs_stat_part,
                     pop_shard, (float*)obs_stat);
  check(hipGetLastError(), "obs_stat_reduce launch");
}

// K policies x M environments, one workgroup per cell (flattened into
// grid.x: K*M may exceed the 65535 cap of grid.y).  episodes == 0 skips
// the per-episode store.
static void launch_eval_matrix(uintptr_t thetas, uintptr_t obs_mu,
                               uintptr_t obs_nu, uintptr_t env_A,
                               uintptr_t env_B, uint32_t seed, uint32_t iter,
                               int horizon, int K, int M, uintptr_t scores,
                               uintptr_t episodes, uintptr_t stream) {
  if (K <= 0 || M <= 0) return;
  const long long cells = (long long)K * (long long)M;
  if (cells > 0x7FFFFFFFLL)
    throw std::runtime_error("es_eval_matrix: K*M exceeds the grid limit");
  if (horizon < 1)
    throw std::runtime_error("es_eval_matrix: horizon must be >= 1");
  hipLaunchKernelGGL(es_eval_matrix, dim3((unsigned)cells), dim3(256), 0,
                     (hipStream_t)stream, (const float*)thetas,
                     (const float*)obs_mu, (const float*)obs_nu,
                     (const float*)env_A, (const float*)env_B, seed, iter,
                     horizon, M, (float*)scores, (float*)episodes);
  check(hipGetLastError(), "es_eval_matrix launch");
}

// Pair-range split of es_grad: enough workgroups to fill the chip (fewer
// chunks for large nparams — bx already provides parallelism).
static int grad_chunks(int pairs, int nparams) {
  const int bx = ((nparams + 3) / 4 + 255) / 256;
  return pairs < 64 ? 1 : (bx >= 32 ? 4 : 32);
}

static void launch_grad(uintptr_t wpair, int pair_begin, int pair_end,
                        uint32_t seed, uint32_t iter, int nparams,
                        uintptr_t grad_part, uintptr_t grad,
                        uintptr_t stream) {
  const int jblocks = (nparams + 3) / 4;
  const int bx = (jblocks + 255) / 256;
  int pairs = pair_end - pair_begin;
  if (pairs <= 0) return;
  // grad_part holds grad_chunks(pairs, nparams) * nparams floats
  const int chunks = grad_chunks(pairs, nparams);
  int per_chunk = (pairs + chunks - 1) / chunks;
  hipLaunchKernelGGL(es_grad, dim3(bx, chunks), dim3(256), 0,
                     (hipStream_t)stream, (const float*)wpair, pair_begin,
                     pair_end, per_chunk, seed, iter, nparams,
                     chunks == 1 ? (float*)grad : (float*)grad_part);
  check(hipGetLastError(), "es_grad launch");
  if (chunks > 1) {
    hipLaunchKernelGGL(es_grad_reduce, dim3((nparams + 255) / 256),
                       dim3(256), 0, (hipStream_t)stream,
                       (const float*)grad_part, chunks, nparams,
                       (float*)grad);
    check(hipGetLastError(), "es_grad_reduce launch");
  }
}

static void launch_centered_rank(uintptr_t f, int n, uintptr_t out,
                                 uintptr_t stream) {
  const int bx = (n + 255) / 256;
  hipLaunchKernelGGL(centered_rank, dim3(bx), dim3(256), 0,
                     (hipStream_t)stream, (const float*)f, n, (float*)out);
  check(hipGetLastError(), "centered_rank launch");
}

// ---- per-pair batched launchers ------------------------------------------
// P pairs per launch.  The pair index is flattened into grid.x for the
// rollout (P*pop outgrows grid.y) and rides grid.y / grid.z elsewhere, so
// P stops at 65535 there; the Python wrappers check all of this first.
#define PAIRS_GRID_MAX 65535

static void check_pairs(const char* what, int P) {
  if (P > PAIRS_GRID_MAX)
    throw std::runtime_error(std::string(what) +
                             ": P exceeds the grid limit");
}

static void launch_rollout_pairs(uintptr_t thetas, double sigma,
                                 uintptr_t seeds, uint32_t iter, int horizon,
                                 int P, int pop, uintptr_t obs_mu,
                                 uintptr_t obs_nu, uintptr_t env_A,
                                 uintptr_t env_B, uintptr_t fitness,
                                 uintptr_t obs_stat_part, uintptr_t obs_stat,
                                 uintptr_t stream) {
  if (P <= 0 || pop <= 0) return;
  check_pairs("es_rollout_mlp_pairs", P);
  const long long blocks = (long long)P * (long long)pop;
  if (blocks > 0x7FFFFFFFLL)
    throw std::runtime_error(
        "es_rollout_mlp_pairs: P*pop exceeds the grid limit");
  if (horizon < 1)
    throw std::runtime_error("es_rollout_mlp_pairs: horizon must be >= 1");
  hipLaunchKernelGGL(es_rollout_mlp_pairs, dim3((unsigned)blocks), dim3(256),
                     0, (hipStream_t)stream, (const float*)thetas,
                     (float)sigma, (const uint32_t*)seeds, iter, horizon,
                     pop, (const float*)obs_mu, (const float*)obs_nu,
                     (const float*)env_A, (const float*)env_B,
                     (float*)fitness, (float*)obs_stat_part,
                     (float*)obs_stat);
  check(hipGetLastError(), "es_rollout_mlp_pairs launch");
  // obs_stat_part is [P][pop][2*OBS]; one block per (stat column, pair)
  hipLaunchKernelGGL(obs_stat_reduce_pairs, dim3(2 * OBS_HOST, P), dim3(256),
                     0, (hipStream_t)stream, (const float*)obs_stat_part,
                     pop, (float*)obs_stat);
  check(hipGetLastError(), "obs_stat_reduce_pairs launch");
}

static void launch_centered_rank_pairs(uintptr_t f, int P, int n,
                                       uintptr_t out, uintptr_t stream) {
  if (P <= 0 || n <= 0) return;
  check_pairs("centered_rank_pairs", P);
  hipLaunchKernelGGL(centered_rank_pairs, dim3((n + 255) / 256, P),
                     dim3(256), 0, (hipStream_t)stream, (const float*)f, n,
                     (float*)out);
  check(hipGetLastError(), "centered_rank_pairs launch");
}

// The split of launch_grad over [0, npairs) for every pair: the same
// chunk count and per_chunk, partials summed in chunk order.  grad_part
// holds P * grad_chunks(npairs, nparams) * nparams floats.
static void launch_grad_pairs(uintptr_t wpair, int P, int npairs,
                              uintptr_t seeds, uint32_t iter, int nparams,
                              uintptr_t grad_part, uintptr_t grad,
                              uintptr_t stream) {
  if (P <= 0 || npairs <= 0) return;
  check_pairs("es_grad_pairs", P);
  const int jblocks = (nparams + 3) / 4;
  const int bx = (jblocks + 255) / 256;
  const int chunks = grad_chunks(npairs, nparams);
  const int per_chunk = (npairs + chunks - 1) / chunks;
  hipLaunchKernelGGL(es_grad_pairs, dim3(bx, chunks, P), dim3(256), 0,
                     (hipStream_t)stream, (const float*)wpair, npairs,
                     per_chunk, (const uint32_t*)seeds, iter, nparams,
                     chunks == 1 ? (float*)grad : (float*)grad_part);
  check(hipGetLastError(), "es_grad_pairs launch");
  if (chunks > 1) {
    hipLaunchKernelGGL(es_grad_reduce_pairs, dim3((nparams + 255) / 256, P),
                       dim3(256), 0, (hipStream_t)stream,
                       (const float*)grad_part, chunks, nparams,
                       (float*)grad);
    check(hipGetLastError(), "es_grad_reduce_pairs launch");
  }
}

// Sort-based rank for large populations: pack order-preserving uint keys,
// stable device radix sort (rocPRIM — AMD-native), scatter ranks.
// Workspace layout: [keys_in][keys_out][vals_in][vals_out][rocprim temp],
// each array 256-byte aligned; caller allocates (torch caching allocator).
static inline uint64_t rank_array_stride(int n) {
  return (((uint64_t)n * 4) + 255) & ~(uint64_t)255;
}

static uint64_t centered_rank_sorted_workspace(int n) {
  size_t temp_bytes = 0;
  check(rocprim::radix_sort_pairs(nullptr, temp_bytes,
                                  (const unsigned*)nullptr,
                                  (unsigned*)nullptr,
                                  (const unsigned*)nullptr,
                                  (unsigned*)nullptr, (size_t)n),
        "radix_sort_pairs size query");
  return 4 * rank_array_stride(n) + (uint64_t)temp_bytes + 256;
}

static void launch_centered_rank_sorted(uintptr_t f, int n, uintptr_t out,
                                        uintptr_t work, uint64_t work_bytes,
                                        uintptr_t stream) {
  const uint64_t stride = rank_array_stride(n);
  if (work_bytes < 4 * stride)
    throw std::runtime_error("centered_rank_sorted workspace too small");
  unsigned* keys_in = (unsigned*)work;
  unsigned* keys_out = (unsigned*)(work + stride);
  unsigned* vals_in = (unsigned*)(work + 2 * stride);
  unsigned* vals_out = (unsigned*)(work + 3 * stride);
  void* temp = (void*)(work + 4 * stride);
  size_t temp_bytes = (size_t)(work_bytes - 4 * stride);
  const int bx = (n + 255) / 256;
  hipLaunchKernelGGL(rank_pack_keys, dim3(bx), dim3(256), 0,
                     (hipStream_t)stream, (const float*)f, n, keys_in,
                     vals_in);
  check(hipGetLastError(), "rank_pack_keys launch");
  check(rocprim::radix_sort_pairs(temp, temp_bytes, keys_in, keys_out,
                                  vals_in, vals_out, (size_t)n, 0, 32,
                                  (hipStream_t)stream),
        "radix_sort_pairs");
  hipLaunchKernelGGL(rank_scatter, dim3(bx), dim3(256), 0,
                     (hipStream_t)stream, vals_out, n, (float*)out);
  check(hipGetLastError(), "rank_scatter launch");
}

static void launch_mlp_forward(uintptr_t theta, uintptr_t x, int batch,
                               uintptr_t logits, uintptr_t stream) {
  const int bx = (batch + ENVS_HOST - 1) / ENVS_HOST;
  hipLaunchKernelGGL(mlp_policy_forward, dim3(bx), dim3(256), 0,
                     (hipStream_t)stream, (const float*)theta,
                     (const float*)x, batch, (float*)logits);
  check(hipGetLastError(), "mlp_policy_forward launch");
}

static void launch_gemm64_probe(uintptr_t a, uintptr_t b, uintptr_t c,
                                uintptr_t stream) {
  hipLaunchKernelGGL(mfma_gemm64_probe, dim3(1), dim3(256), 0,
                     (hipStream_t)stream, (const float*)a, (const float*)b,
                     (float*)c);
  check(hipGetLastError(), "mfma_gemm64_probe launch");
}

// p0, p1: [4][64] partials; out_shfl, out_swap: [64][2].  One wave.
static void launch_logits_reduce_probe(uintptr_t p0, uintptr_t p1,
                                       uintptr_t out_shfl,
                                       uintptr_t out_swap,
                                       uintptr_t stream) {
  hipLaunchKernelGGL(logits_reduce_probe, dim3(1), dim3(64), 0,
                     (hipStream_t)stream, (const float*)p0,
                     (const float*)p1, (float*)out_shfl, (float*)out_swap);
  check(hipGetLastError(), "logits_reduce_probe launch");
}

// ---- novelty-search launchers --------------------------------------------
// The limits of bc_knn_novelty (ns_kernels.hip): neighbours kept per query
// and archive rows per LDS tile.
#define BC_KNN_MAX_HOST 16
#define BC_KNN_TILE_HOST 1024

// launch_rollout with a BC per member; final_states == 0 skips that store.
static void launch_rollout_bc(uintptr_t theta, double sigma, uint32_t seed,
                              uint32_t iter, int horizon, int member_offset,
                              int pop_shard, uintptr_t obs_mu,
                              uintptr_t obs_nu, uintptr_t env_A,
                              uintptr_t env_B, uintptr_t fitness,
                              uintptr_t obs_stat_part, uintptr_t obs_stat,
                              uintptr_t bc, uintptr_t final_states,
                              uintptr_t stream) {
  if (pop_shard <= 0) return;
  if (horizon < 1)
    throw std::runtime_error("es_rollout_mlp_bc: horizon must be >= 1");
  hipLaunchKernelGGL(es_rollout_mlp_bc, dim3(pop_shard), dim3(256), 0,
                     (hipStream_t)stream, (const float*)theta, (float)sigma,
                     seed, iter, horizon, member_offset,
                     (const float*)obs_mu, (const float*)obs_nu,
                     (const float*)env_A, (const float*)env_B,
                     (float*)fitness, (float*)obs_stat_part,
                     (float*)obs_stat, (float*)bc, (float*)final_states);
  check(hipGetLastError(), "es_rollout_mlp_bc launch");
  hipLaunchKernelGGL(obs_stat_reduce, dim3(2 * OBS_HOST), dim3(256), 0,
                     (hipStream_t)stream, (const float*)obs_stat_part,
                     pop_shard, (float*)obs_stat);
  check(hipGetLastError(), "obs_stat_reduce launch");
}

// launch_eval_matrix with a BC per cell; episodes / final_states == 0 skip
// those stores.
static void launch_eval_bc(uintptr_t thetas, uintptr_t obs_mu,
                           uintptr_t obs_nu, uintptr_t env_A,
                           uintptr_t env_B, uint32_t seed, uint32_t iter,
                           int horizon, int K, int M, uintptr_t scores,
                           uintptr_t episodes, uintptr_t bc,
                           uintptr_t final_states, uintptr_t stream) {
  if (K <= 0 || M <= 0) return;
  const long long cells = (long long)K * (long long)M;
  if (cells > 0x7FFFFFFFLL)
    throw std::runtime_error("es_eval_bc: K*M exceeds the grid limit");
  if (horizon < 1)
    throw std::runtime_error("es_eval_bc: horizon must be >= 1");
  hipLaunchKernelGGL(es_eval_bc, dim3((unsigned)cells), dim3(256), 0,
                     (hipStream_t)stream, (const float*)thetas,
                     (const float*)obs_mu, (const float*)obs_nu,
                     (const float*)env_A, (const float*)env_B, seed, iter,
                     horizon, M, (float*)scores, (float*)episodes,
                     (float*)bc, (float*)final_states);
  check(hipGetLastError(), "es_eval_bc launch");
}

// N queries against R archive rows, one thread per query; knn_d2 == 0
// skips the neighbour store.
static void launch_bc_knn_novelty(uintptr_t bc, int N, uintptr_t archive,
                                  int R, int k, uintptr_t novelty,
                                  uintptr_t knn_d2, uintptr_t stream) {
  if (N < 1 || R < 1 || k < 1 || k > BC_KNN_MAX_HOST || k > R)
    throw std::runtime_error("bc_knn_novelty: bad N, R or k");
  hipLaunchKernelGGL(bc_knn_novelty, dim3((unsigned)((N + 255) / 256)),
                     dim3(256), 0, (hipStream_t)stream, (const float*)bc, N,
                     (const float*)archive, R, k, (float*)novelty,
                     (float*)knn_d2);
  check(hipGetLastError(), "bc_knn_novelty launch");
}

// ---- separable-NES launchers ---------------------------------------------

// launch_rollout with a device vector sigma[NPARAMS] in place of the scalar.
static void launch_rollout_sigma(uintptr_t theta, uintptr_t sigma,
                                 uint32_t seed, uint32_t iter, int horizon,
                                 int member_offset, int pop_shard,
                                 uintptr_t obs_mu, uintptr_t obs_nu,
                                 uintptr_t env_A, uintptr_t env_B,
                                 uintptr_t fitness, uintptr_t obs_stat_part,
                                 uintptr_t obs_stat, uintptr_t stream) {
  if (pop_shard <= 0) return;
  if (horizon < 1)
    throw std::runtime_error("es_rollout_mlp_sigma: horizon must be >= 1");
  hipLaunchKernelGGL(es_rollout_mlp_sigma, dim3(pop_shard), dim3(256), 0,
                     (hipStream_t)stream, (const float*)theta,
                     (const float*)sigma, seed, iter, horizon, member_offset,
                     (const float*)obs_mu, (const float*)obs_nu,
                     (const float*)env_A, (const float*)env_B,
                     (float*)fitness, (float*)obs_stat_part,
                     (float*)obs_stat);
  check(hipGetLastError(), "es_rollout_mlp_sigma launch");
  hipLaunchKernelGGL(obs_stat_reduce, dim3(2 * OBS_HOST), dim3(256), 0,
                     (hipStream_t)stream, (const float*)obs_stat_part,
                     pop_shard, (float*)obs_stat);
  check(hipGetLastError(), "obs_stat_reduce launch");
}

// The split of launch_grad with two rows per chunk: grad is [2][nparams]
// (g_mu, g_sig), grad_part holds grad_chunks(pairs, nparams) * 2 * nparams
// floats, and es_grad_reduce sums the partials over 2*nparams columns in
// chunk order.
static void launch_grad_sigma(uintptr_t wdiff, uintptr_t wsum,
                              int pair_begin, int pair_end, uint32_t seed,
                              uint32_t iter, int nparams,
                              uintptr_t grad_part, uintptr_t grad,
                              uintptr_t stream) {
  const int jblocks = (nparams + 3) / 4;
  const int bx = (jblocks + 255) / 256;
  const int pairs = pair_end - pair_begin;
  if (pairs <= 0) return;
  if (nparams < 1 || nparams > 0x3FFFFFFF)
    throw std::runtime_error("es_grad_sigma: bad nparams");
  const int chunks = grad_chunks(pairs, nparams);
  const int per_chunk = (pairs + chunks - 1) / chunks;
  hipLaunchKernelGGL(es_grad_sigma, dim3(bx, chunks), dim3(256), 0,
                     (hipStream_t)stream, (const float*)wdiff,
                     (const float*)wsum, pair_begin, pair_end, per_chunk,
                     seed, iter, nparams,
                     chunks == 1 ? (float*)grad : (float*)grad_part);
  check(hipGetLastError(), "es_grad_sigma launch");
  if (chunks > 1) {
    hipLaunchKernelGGL(es_grad_reduce, dim3((2 * nparams + 255) / 256),
                       dim3(256), 0, (hipStream_t)stream,
                       (const float*)grad_part, chunks, 2 * nparams,
                       (float*)grad);
    check(hipGetLastError(), "es_grad_reduce launch");
  }
}

// ---- Deep GA launchers ------------------------------------------------------
// ga_truncate counts over all n per thread and stops at 65536 members;
// ga_survivors and ga_decode carry the row in grid.y.
#define GA_TRUNCATE_MAX_HOST 65536
#define GA_ROWS_MAX_HOST 65535

static void launch_ga_parents(uint32_t seed, uint32_t gen, int pop,
                              int n_elite, int T_cur, uintptr_t parent_idx,
                              uintptr_t slot, uintptr_t stream) {
  if (pop < 1 || T_cur < 1 || n_elite < 0 || n_elite > T_cur)
    throw std::runtime_error("ga_parents: bad pop, n_elite or T_cur");
  hipLaunchKernelGGL(ga_parents, dim3((unsigned)((pop + 255) / 256)),
                     dim3(256), 0, (hipStream_t)stream, seed, gen, pop,
                     n_elite, (uint32_t)T_cur, (int*)parent_idx, (int*)slot);
  check(hipGetLastError(), "ga_parents launch");
}

// launch_rollout with a parent row and a draw per member.
static void launch_ga_rollout(uintptr_t parents, uintptr_t parent_idx,
                              uintptr_t slot, double sigma, uint32_t seed,
                              uint32_t gen, int horizon, int pop,
                              uintptr_t obs_mu, uintptr_t obs_nu,
                              uintptr_t env_A, uintptr_t env_B,
                              uintptr_t fitness, uintptr_t obs_stat_part,
                              uintptr_t obs_stat, uintptr_t stream) {
  if (pop < 1) throw std::runtime_error("ga_rollout_mlp: pop must be >= 1");
  if (horizon < 1)
    throw std::runtime_error("ga_rollout_mlp: horizon must be >= 1");
  hipLaunchKernelGGL(ga_rollout_mlp, dim3(pop), dim3(256), 0,
                     (hipStream_t)stream, (const float*)parents,
                     (const int*)parent_idx, (const int*)slot, (float)sigma,
                     seed, gen, horizon, (const float*)obs_mu,
                     (const float*)obs_nu, (const float*)env_A,
                     (const float*)env_B, (float*)fitness,
                     (float*)obs_stat_part, (float*)obs_stat);
  check(hipGetLastError(), "ga_rollout_mlp launch");
  hipLaunchKernelGGL(obs_stat_reduce, dim3(2 * OBS_HOST), dim3(256), 0,
                     (hipStream_t)stream, (const float*)obs_stat_part, pop,
                     (float*)obs_stat);
  check(hipGetLastError(), "obs_stat_reduce launch");
}

static void launch_ga_truncate(uintptr_t f, int n, int T, uintptr_t order,
                               uintptr_t stream) {
  if (n < 2 || n > GA_TRUNCATE_MAX_HOST || T < 1 || T > n)
    throw std::runtime_error("ga_truncate: bad n or T");
  hipLaunchKernelGGL(ga_truncate, dim3((unsigned)((n + 255) / 256)),
                     dim3(256), 0, (hipStream_t)stream, (const float*)f, n,
                     T, (int*)order);
  check(hipGetLastError(), "ga_truncate launch");
}

static void launch_ga_survivors(uintptr_t parents, uintptr_t parent_idx,
                                uintptr_t slot, uintptr_t order, int T,
                                double sigma, uint32_t seed, uint32_t gen,
                                uintptr_t new_parents, uintptr_t stream) {
  if (T < 1 || T > GA_ROWS_MAX_HOST)
    throw std::runtime_error("ga_survivors: bad T");
  if (parents == new_parents)
    throw std::runtime_error("ga_survivors: new_parents aliases parents");
  const int bx = ((NPARAMS_HOST + 3) / 4 + 255) / 256;
  hipLaunchKernelGGL(ga_survivors, dim3(bx, T), dim3(256), 0,
                     (hipStream_t)stream, (const float*)parents,
                     (const int*)parent_idx, (const int*)slot,
                     (const int*)order, (float)sigma, seed, gen,
                     (float*)new_parents);
  check(hipGetLastError(), "ga_survivors launch");
}

static void launch_ga_decode(uintptr_t theta0, uintptr_t lineage, int N,
                             int G, double sigma, uint32_t seed,
                             uintptr_t thetas, uintptr_t stream) {
  if (N < 1 || N > GA_ROWS_MAX_HOST || G < 0)
    throw std::runtime_error("ga_decode: bad N or G");
  const int bx = ((NPARAMS_HOST + 3) / 4 + 255) / 256;
  hipLaunchKernelGGL(ga_decode, dim3(bx, N), dim3(256), 0,
                     (hipStream_t)stream, (const float*)theta0,
                     (const int*)lineage, G, (float)sigma, seed,
                     (float*)thetas);
  check(hipGetLastError(), "ga_decode launch");
}

// ---- safe-mutation launchers -------------------------------------------------
static void launch_sm_steps(uintptr_t thetas, uintptr_t probe, int T,
                            double sigma, double s_min, int mode,
                            uintptr_t steps, uintptr_t sens,
                            uintptr_t stream) {
  if (T < 1 || T > GA_ROWS_MAX_HOST)
    throw std::runtime_error("sm_steps: bad T");
  if (mode != 0 && mode != 1) throw std::runtime_error("sm_steps: bad mode");
  if (!(sigma >= 0.0) || !(s_min > 0.0))
    throw std::runtime_error("sm_steps: bad sigma or s_min");
  hipLaunchKernelGGL(sm_steps, dim3(T), dim3(256), 0, (hipStream_t)stream,
                     (const float*)thetas, (const float*)probe, (float)sigma,
                     (float)s_min, mode, (float*)steps, (float*)sens);
  check(hipGetLastError(), "sm_steps launch");
}

// launch_ga_rollout with a step row per parent.
static void launch_ga_rollout_sm(uintptr_t parents, uintptr_t steps,
                                 uintptr_t parent_idx, uintptr_t slot,
                                 uint32_t seed, uint32_t gen, int horizon,
                                 int pop, uintptr_t obs_mu, uintptr_t obs_nu,
                                 uintptr_t env_A, uintptr_t env_B,
                                 uintptr_t fitness, uintptr_t obs_stat_part,
                                 uintptr_t obs_stat, uintptr_t stream) {
  if (pop < 1)
    throw std::runtime_error("ga_rollout_mlp_sm: pop must be >= 1");
  if (horizon < 1)
    throw std::runtime_error("ga_rollout_mlp_sm: horizon must be >= 1");
  hipLaunchKernelGGL(ga_rollout_mlp_sm, dim3(pop), dim3(256), 0,
                     (hipStream_t)stream, (const float*)parents,
                     (const float*)steps, (const int*)parent_idx,
                     (const int*)slot, seed, gen, horizon,
                     (const float*)obs_mu, (const float*)obs_nu,
                     (const float*)env_A, (const float*)env_B,
                     (float*)fitness, (float*)obs_stat_part,
                     (float*)obs_stat);
  check(hipGetLastError(), "ga_rollout_mlp_sm launch");
  hipLaunchKernelGGL(obs_stat_reduce, dim3(2 * OBS_HOST), dim3(256), 0,
                     (hipStream_t)stream, (const float*)obs_stat_part, pop,
                     (float*)obs_stat);
  check(hipGetLastError(), "obs_stat_reduce launch");
}

static void launch_ga_survivors_sm(uintptr_t parents, uintptr_t steps,
                                   uintptr_t parent_idx, uintptr_t slot,
                                   uintptr_t order, int T, uint32_t seed,
                                   uint32_t gen, uintptr_t new_parents,
                                   uintptr_t stream) {
  if (T < 1 || T > GA_ROWS_MAX_HOST)
    throw std::runtime_error("ga_survivors_sm: bad T");
  if (parents == new_parents || steps == new_parents)
    throw std::runtime_error(
        "ga_survivors_sm: new_parents aliases parents or steps");
  const int bx = ((NPARAMS_HOST + 3) / 4 + 255) / 256;
  hipLaunchKernelGGL(ga_survivors_sm, dim3(bx, T), dim3(256), 0,
                     (hipStream_t)stream, (const float*)parents,
                     (const float*)steps, (const int*)parent_idx,
                     (const int*)slot, (const int*)order, seed, gen,
                     (float*)new_parents);
  check(hipGetLastError(), "ga_survivors_sm launch");
}

// ---- MAP-Elites launchers ---------------------------------------------------
// The archive's rows ride grid.y of ga_survivors and ga_decode with the root
// row behind them, so C + 1 <= GA_ROWS_MAX.
#define ME_CELLS_MAX_HOST (GA_ROWS_MAX_HOST - 1)

static void launch_me_parents(uint32_t seed, uint32_t gen, int pop,
                              uintptr_t filled_idx, uintptr_t n_filled,
                              int root_row, uintptr_t parent_idx,
                              uintptr_t slot, uintptr_t stream) {
  if (pop < 1 || root_row < 0)
    throw std::runtime_error("me_parents: bad pop or root_row");
  hipLaunchKernelGGL(me_parents, dim3((unsigned)((pop + 255) / 256)),
                     dim3(256), 0, (hipStream_t)stream, seed, gen, pop,
                     (const int*)filled_idx, (const int*)n_filled, root_row,
                     (int*)parent_idx, (int*)slot);
  check(hipGetLastError(), "me_parents launch");
}

// launch_ga_rollout with a BC per member.
static void launch_ga_rollout_bc(uintptr_t parents, uintptr_t parent_idx,
                                 uintptr_t slot, double sigma, uint32_t seed,
                                 uint32_t gen, int horizon, int pop,
                                 uintptr_t obs_mu, uintptr_t obs_nu,
                                 uintptr_t env_A, uintptr_t env_B,
                                 uintptr_t fitness, uintptr_t obs_stat_part,
                                 uintptr_t obs_stat, uintptr_t bc,
                                 uintptr_t final_states, uintptr_t stream) {
  if (pop < 1)
    throw std::runtime_error("ga_rollout_mlp_bc: pop must be >= 1");
  if (horizon < 1)
    throw std::runtime_error("ga_rollout_mlp_bc: horizon must be >= 1");
  hipLaunchKernelGGL(ga_rollout_mlp_bc, dim3(pop), dim3(256), 0,
                     (hipStream_t)stream, (const float*)parents,
                     (const int*)parent_idx, (const int*)slot, (float)sigma,
                     seed, gen, horizon, (const float*)obs_mu,
                     (const float*)obs_nu, (const float*)env_A,
                     (const float*)env_B, (float*)fitness,
                     (float*)obs_stat_part, (float*)obs_stat, (float*)bc,
                     (float*)final_states);
  check(hipGetLastError(), "ga_rollout_mlp_bc launch");
  hipLaunchKernelGGL(obs_stat_reduce, dim3(2 * OBS_HOST), dim3(256), 0,
                     (hipStream_t)stream, (const float*)obs_stat_part, pop,
                     (float*)obs_stat);
  check(hipGetLastError(), "obs_stat_reduce launch");
}

// best[C] is 64-bit scratch, zeroed here on the stream before me_assign.
static void launch_me_insert(uintptr_t fitness, uintptr_t bc, int pop,
                             py::tuple bins, py::tuple lo, py::tuple inv,
                             uintptr_t arch_fitness, uintptr_t arch_bc,
                             uintptr_t arch_filled, uintptr_t best,
                             uintptr_t cell, uintptr_t winner,
                             uintptr_t order, uintptr_t stream) {
  if (bins.size() != 4 || lo.size() != 4 || inv.size() != 4)
    throw std::runtime_error("me_insert: the grid has 4 dimensions");
  MeGrid grid;
  long long C = 1;
  for (int d = 0; d < 4; ++d) {
    grid.bins[d] = bins[d].cast<int>();
    grid.lo[d] = lo[d].cast<float>();
    grid.inv[d] = inv[d].cast<float>();
    if (grid.bins[d] < 1 || grid.bins[d] > ME_CELLS_MAX_HOST)
      throw std::runtime_error("me_insert: bad bins");
    C *= grid.bins[d];
    if (C > ME_CELLS_MAX_HOST)
      throw std::runtime_error("me_insert: too many cells");
  }
  if (pop < 1 || pop > GA_TRUNCATE_MAX_HOST)
    throw std::runtime_error("me_insert: bad pop");
  check(hipMemsetAsync((void*)best, 0, (size_t)C * 8, (hipStream_t)stream),
        "me_insert memset");
  hipLaunchKernelGGL(me_assign, dim3((unsigned)((pop + 255) / 256)),
                     dim3(256), 0, (hipStream_t)stream,
                     (const float*)fitness, (const float*)bc, pop, grid,
                     (int*)cell, (unsigned long long*)best);
  check(hipGetLastError(), "me_assign launch");
  hipLaunchKernelGGL(me_commit, dim3((unsigned)((C + 1 + 255) / 256)),
                     dim3(256), 0, (hipStream_t)stream,
                     (const float*)fitness, (const float*)bc, pop, (int)C,
                     (const unsigned long long*)best, (float*)arch_fitness,
                     (float*)arch_bc, (int*)arch_filled, (int*)winner,
                     (int*)order);
  check(hipGetLastError(), "me_commit launch");
}

static void launch_me_compact(uintptr_t arch_filled, int C,
                              uintptr_t filled_idx, uintptr_t n_filled,
                              uintptr_t stream) {
  if (C < 1 || C > ME_CELLS_MAX_HOST)
    throw std::runtime_error("me_compact: bad C");
  hipLaunchKernelGGL(me_compact, dim3(1), dim3(1024), 0, (hipStream_t)stream,
                     (const int*)arch_filled, C, (int*)filled_idx,
                     (int*)n_filled);
  check(hipGetLastError(), "me_compact launch");
}

// ---- conv pipeline launchers ---------------------------------------------

static void launch_perturb(uintptr_t theta, int nparams, int np_pad,
                           double sigma, uint32_t seed, uintptr_t iterp,
                           int member_offset, int pop, uintptr_t wpert,
                           uintptr_t w3_fp8, uintptr_t w1_fp8,
                           uintptr_t stream) {
  if ((member_offset | pop) & 1)
    throw std::runtime_error(
        "es_perturb needs pair-aligned member_offset/pop");
  const int bx = 64;  // grid-stride over param blocks; grid.y = PAIRS
  hipLaunchKernelGGL(es_perturb, dim3(bx, pop / 2), dim3(256), 0,
                     (hipStream_t)stream, (const float*)theta, nparams,
                     np_pad, (float)sigma, seed, (const uint32_t*)iterp,
                     member_offset, (__hip_bfloat16*)wpert,
                     (unsigned char*)w3_fp8, (unsigned char*)w1_fp8);
  check(hipGetLastError(), "es_perturb launch");
}

static void launch_conv_env_init(uint32_t seed, uintptr_t iterp,
                                 int nmembers, uintptr_t state,
                                 uintptr_t racc, uintptr_t stream) {
  const int n = nmembers * 16;
  hipLaunchKernelGGL(conv_env_init, dim3((n + 255) / 256), dim3(256), 0,
                     (hipStream_t)stream, seed, (const uint32_t*)iterp,
                     nmembers, (float*)state, (float*)racc);
  check(hipGetLastError(), "conv_env_init launch");
}

static void launch_conv_noisegen(uint32_t seed, uintptr_t iterp, uint32_t t,
                                 int nenv, uintptr_t znoise,
                                 uintptr_t stream) {
  // flattened (env, position-quad) grid; 7056/4 quads per env
  const int total = nenv * (84 * 84 / 4);
  hipLaunchKernelGGL(conv_noisegen, dim3((total + 255) / 256), dim3(256), 0,
                     (hipStream_t)stream, seed, (const uint32_t*)iterp, t,
                     (unsigned char*)znoise);
  check(hipGetLastError(), "conv_noisegen launch");
}

// One launcher per MFMA layer, so the layer tests can drive each kernel
// on its own; conv_forward is the three of them in order.
static void launch_conv_layer1(uintptr_t wpert, uintptr_t w1_fp8,
                               uintptr_t state, uintptr_t gtab,
                               uintptr_t znoise, uintptr_t act1,
                               int nmembers, uintptr_t stream) {
  const int nenv = nmembers * 16;
  hipLaunchKernelGGL(conv_layer1, dim3(nenv), dim3(256), 0,
                     (hipStream_t)stream, (const __hip_bfloat16*)wpert,
                     (const unsigned char*)w1_fp8, (const float*)state,
                     (const __hip_bfloat16*)gtab,
                     (const unsigned char*)znoise, nenv,
                     (__hip_bfloat16*)act1);
  check(hipGetLastError(), "conv_layer1 launch");
}

static void launch_conv_layer2(uintptr_t wpert, uintptr_t act1,
                               uintptr_t act2, int nmembers,
                               uintptr_t stream) {
  const int nenv = nmembers * 16;
  hipLaunchKernelGGL(conv_layer2, dim3(nenv), dim3(256), 0,
                     (hipStream_t)stream, (const __hip_bfloat16*)wpert,
                     (const __hip_bfloat16*)act1, nenv,
                     (unsigned char*)act2);
  check(hipGetLastError(), "conv_layer2 launch");
}

static void launch_conv_fc(uintptr_t wpert, uintptr_t w3_fp8,
                           uintptr_t act2, uintptr_t act3, int nmembers,
                           uintptr_t stream) {
  hipLaunchKernelGGL(conv_fc, dim3(nmembers, 4), dim3(256), 0,
                     (hipStream_t)stream, (const __hip_bfloat16*)wpert,
                     (const unsigned char*)w3_fp8,
                     (const unsigned char*)act2, nmembers,
                     (__hip_bfloat16*)act3);
  check(hipGetLastError(), "conv_fc launch");
}

static void launch_conv_forward(uintptr_t wpert, uintptr_t w3_fp8,
                                uintptr_t w1_fp8, uintptr_t state,
                                uintptr_t gtab, uintptr_t znoise,
                                uintptr_t act1, uintptr_t act2,
                                uintptr_t act3, int nmembers,
                                uintptr_t stream) {
  launch_conv_layer1(wpert, w1_fp8, state, gtab, znoise, act1, nmembers,
                     stream);
  launch_conv_layer2(wpert, act1, act2, nmembers, stream);
  launch_conv_fc(wpert, w3_fp8, act2, act3, nmembers, stream);
}

static void launch_conv_head_env(uintptr_t wpert, uintptr_t act3,
                                 int nmembers, uintptr_t env_A,
                                 uintptr_t env_B, uintptr_t state,
                                 uintptr_t racc, uintptr_t stream) {
  hipLaunchKernelGGL(conv_head_env, dim3(nmembers), dim3(256), 0,
                     (hipStream_t)stream, (const __hip_bfloat16*)wpert,
                     (const __hip_bfloat16*)act3, nmembers,
                     (const float*)env_A, (const float*)env_B,
                     (float*)state, (float*)racc);
  check(hipGetLastError(), "conv_head_env launch");
}

// scores[K][M] -> codes[M][Kpad]: one block per 16 columns.  The caps are
// those of the kernels' LDS arrays (poet_kernels.hip).
static void launch_pata_ec_codes(uintptr_t scores, int K, int M, int Kpad,
                                 double lo, double hi, uintptr_t codes,
                                 uintptr_t stream) {
  if (K < 2 || K > 512 || M < 1 || Kpad != (K + 7) / 8 * 8)
    throw std::runtime_error("pata_ec_codes: bad K, M or Kpad");
  hipLaunchKernelGGL(pata_ec_codes, dim3((unsigned)((M + 15) / 16)),
                     dim3(256), 0, (hipStream_t)stream,
                     (const float*)scores, K, M, Kpad, (float)lo, (float)hi,
                     (int16_t*)codes);
  check(hipGetLastError(), "pata_ec_codes launch");
}

// codes rows [n_ref, n_ref + Q) against rows [0, n_ref): 4 queries per
// block; k is already min(k, n_ref).
static void launch_pata_ec_knn(uintptr_t codes, int Kpad, int K, int n_ref,
                               int Q, int k, uintptr_t knn_d2,
                               uintptr_t novelty, uintptr_t stream) {
  if (K < 2 || K > 512 || Kpad != (K + 7) / 8 * 8 || n_ref < 1 || Q < 1 ||
      k < 1 || k > 64 || k > n_ref)
    throw std::runtime_error("pata_ec_knn: bad K, Kpad, n_ref, Q or k");
  hipLaunchKernelGGL(pata_ec_knn, dim3((unsigned)((Q + 3) / 4)), dim3(256),
                     0, (hipStream_t)stream, (const int16_t*)codes, Kpad, K,
                     n_ref, Q, k, (int*)knn_d2, (float*)novelty);
  check(hipGetLastError(), "pata_ec_knn launch");
}

PYBIND11_MODULE(_ops, m) {
  m.doc() = "fiber_amd CDNA4 ES kernels (gfx950)";
  m.attr("NPARAMS") = NPARAMS_HOST;
  m.attr("ENVS_PER_MEMBER") = ENVS_HOST;
  m.def("es_rollout_mlp", &launch_rollout, py::arg("theta"),
        py::arg("sigma"), py::arg("seed"), py::arg("iter"),
        py::arg("horizon"), py::arg("member_offset"), py::arg("pop_shard"),
        py::arg("obs_mu"), py::arg("obs_nu"), py::arg("env_A"),
        py::arg("env_B"), py::arg("fitness"), py::arg("obs_stat_part"),
        py::arg("obs_stat"), py::arg("stream"));
  m.def("es_eval_matrix", &launch_eval_matrix, py::arg("thetas"),
        py::arg("obs_mu"), py::arg("obs_nu"), py::arg("env_A"),
        py::arg("env_B"), py::arg("seed"), py::arg("iter"),
        py::arg("horizon"), py::arg("K"), py::arg("M"), py::arg("scores"),
        py::arg("episodes"), py::arg("stream"));
  m.def("es_grad", &launch_grad, py::arg("wpair"), py::arg("pair_begin"),
        py::arg("pair_end"), py::arg("seed"), py::arg("iter"),
        py::arg("nparams"), py::arg("grad_part"), py::arg("grad"),
        py::arg("stream"));
  m.def("es_grad_chunks", &grad_chunks, py::arg("pairs"),
        py::arg("nparams"));
  m.def("centered_rank", &launch_centered_rank, py::arg("f"), py::arg("n"),
        py::arg("out"), py::arg("stream"));
  m.def("es_rollout_mlp_pairs", &launch_rollout_pairs, py::arg("thetas"),
        py::arg("sigma"), py::arg("seeds"), py::arg("iter"),
        py::arg("horizon"), py::arg("P"), py::arg("pop"), py::arg("obs_mu"),
        py::arg("obs_nu"), py::arg("env_A"), py::arg("env_B"),
        py::arg("fitness"), py::arg("obs_stat_part"), py::arg("obs_stat"),
        py::arg("stream"));
  m.def("centered_rank_pairs", &launch_centered_rank_pairs, py::arg("f"),
        py::arg("P"), py::arg("n"), py::arg("out"), py::arg("stream"));
  m.def("es_grad_pairs", &launch_grad_pairs, py::arg("wpair"), py::arg("P"),
        py::arg("npairs"), py::arg("seeds"), py::arg("iter"),
        py::arg("nparams"), py::arg("grad_part"), py::arg("grad"),
        py::arg("stream"));
  m.attr("BC_KNN_MAX") = BC_KNN_MAX_HOST;
  m.attr("BC_KNN_TILE") = BC_KNN_TILE_HOST;
  m.def("es_rollout_mlp_bc", &launch_rollout_bc, py::arg("theta"),
        py::arg("sigma"), py::arg("seed"), py::arg("iter"),
        py::arg("horizon"), py::arg("member_offset"), py::arg("pop_shard"),
        py::arg("obs_mu"), py::arg("obs_nu"), py::arg("env_A"),
        py::arg("env_B"), py::arg("fitness"), py::arg("obs_stat_part"),
        py::arg("obs_stat"), py::arg("bc"), py::arg("final_states"),
        py::arg("stream"));
  m.def("es_eval_bc", &launch_eval_bc, py::arg("thetas"), py::arg("obs_mu"),
        py::arg("obs_nu"), py::arg("env_A"), py::arg("env_B"),
        py::arg("seed"), py::arg("iter"), py::arg("horizon"), py::arg("K"),
        py::arg("M"), py::arg("scores"), py::arg("episodes"), py::arg("bc"),
        py::arg("final_states"), py::arg("stream"));
  m.def("bc_knn_novelty", &launch_bc_knn_novelty, py::arg("bc"),
        py::arg("N"), py::arg("archive"), py::arg("R"), py::arg("k"),
        py::arg("novelty"), py::arg("knn_d2"), py::arg("stream"));
  m.def("es_rollout_mlp_sigma", &launch_rollout_sigma, py::arg("theta"),
        py::arg("sigma"), py::arg("seed"), py::arg("iter"),
        py::arg("horizon"), py::arg("member_offset"), py::arg("pop_shard"),
        py::arg("obs_mu"), py::arg("obs_nu"), py::arg("env_A"),
        py::arg("env_B"), py::arg("fitness"), py::arg("obs_stat_part"),
        py::arg("obs_stat"), py::arg("stream"));
  m.def("es_grad_sigma", &launch_grad_sigma, py::arg("wdiff"),
        py::arg("wsum"), py::arg("pair_begin"), py::arg("pair_end"),
        py::arg("seed"), py::arg("iter"), py::arg("nparams"),
        py::arg("grad_part"), py::arg("grad"), py::arg("stream"));
  m.attr("GA_TRUNCATE_MAX") = GA_TRUNCATE_MAX_HOST;
  m.attr("GA_ROWS_MAX") = GA_ROWS_MAX_HOST;
  m.def("ga_parents", &launch_ga_parents, py::arg("seed"), py::arg("gen"),
        py::arg("pop"), py::arg("n_elite"), py::arg("T_cur"),
        py::arg("parent_idx"), py::arg("slot"), py::arg("stream"));
  m.def("ga_rollout_mlp", &launch_ga_rollout, py::arg("parents"),
        py::arg("parent_idx"), py::arg("slot"), py::arg("sigma"),
        py::arg("seed"), py::arg("gen"), py::arg("horizon"), py::arg("pop"),
        py::arg("obs_mu"), py::arg("obs_nu"), py::arg("env_A"),
        py::arg("env_B"), py::arg("fitness"), py::arg("obs_stat_part"),
        py::arg("obs_stat"), py::arg("stream"));
  m.def("ga_truncate", &launch_ga_truncate, py::arg("f"), py::arg("n"),
        py::arg("T"), py::arg("order"), py::arg("stream"));
  m.def("ga_survivors", &launch_ga_survivors, py::arg("parents"),
        py::arg("parent_idx"), py::arg("slot"), py::arg("order"),
        py::arg("T"), py::arg("sigma"), py::arg("seed"), py::arg("gen"),
        py::arg("new_parents"), py::arg("stream"));
  m.def("ga_decode", &launch_ga_decode, py::arg("theta0"),
        py::arg("lineage"), py::arg("N"), py::arg("G"), py::arg("sigma"),
        py::arg("seed"), py::arg("thetas"), py::arg("stream"));
  m.def("sm_steps", &launch_sm_steps, py::arg("thetas"), py::arg("probe"),
        py::arg("T"), py::arg("sigma"), py::arg("s_min"), py::arg("mode"),
        py::arg("steps"), py::arg("sens"), py::arg("stream"));
  m.def("ga_rollout_mlp_sm", &launch_ga_rollout_sm, py::arg("parents"),
        py::arg("steps"), py::arg("parent_idx"), py::arg("slot"),
        py::arg("seed"), py::arg("gen"), py::arg("horizon"), py::arg("pop"),
        py::arg("obs_mu"), py::arg("obs_nu"), py::arg("env_A"),
        py::arg("env_B"), py::arg("fitness"), py::arg("obs_stat_part"),
        py::arg("obs_stat"), py::arg("stream"));
  m.def("ga_survivors_sm", &launch_ga_survivors_sm, py::arg("parents"),
        py::arg("steps"), py::arg("parent_idx"), py::arg("slot"),
        py::arg("order"), py::arg("T"), py::arg("seed"), py::arg("gen"),
        py::arg("new_parents"), py::arg("stream"));
  m.attr("ME_CELLS_MAX") = ME_CELLS_MAX_HOST;
  m.def("me_parents", &launch_me_parents, py::arg("seed"), py::arg("gen"),
        py::arg("pop"), py::arg("filled_idx"), py::arg("n_filled"),
        py::arg("root_row"), py::arg("parent_idx"), py::arg("slot"),
        py::arg("stream"));
  m.def("ga_rollout_mlp_bc", &launch_ga_rollout_bc, py::arg("parents"),
        py::arg("parent_idx"), py::arg("slot"), py::arg("sigma"),
        py::arg("seed"), py::arg("gen"), py::arg("horizon"), py::arg("pop"),
        py::arg("obs_mu"), py::arg("obs_nu"), py::arg("env_A"),
        py::arg("env_B"), py::arg("fitness"), py::arg("obs_stat_part"),
        py::arg("obs_stat"), py::arg("bc"), py::arg("final_states"),
        py::arg("stream"));
  m.def("me_insert", &launch_me_insert, py::arg("fitness"), py::arg("bc"),
        py::arg("pop"), py::arg("bins"), py::arg("lo"), py::arg("inv"),
        py::arg("arch_fitness"), py::arg("arch_bc"), py::arg("arch_filled"),
        py::arg("best"), py::arg("cell"), py::arg("winner"),
        py::arg("order"), py::arg("stream"));
  m.def("me_compact", &launch_me_compact, py::arg("arch_filled"),
        py::arg("C"), py::arg("filled_idx"), py::arg("n_filled"),
        py::arg("stream"));
  m.def("pata_ec_codes", &launch_pata_ec_codes, py::arg("scores"),
        py::arg("K"), py::arg("M"), py::arg("Kpad"), py::arg("lo"),
        py::arg("hi"), py::arg("codes"), py::arg("stream"));
  m.def("pata_ec_knn", &launch_pata_ec_knn, py::arg("codes"),
        py::arg("Kpad"), py::arg("K"), py::arg("n_ref"), py::arg("Q"),
        py::arg("k"), py::arg("knn_d2"), py::arg("novelty"),
        py::arg("stream"));
  m.def("centered_rank_sorted_workspace", &centered_rank_sorted_workspace,
        py::arg("n"));
  m.def("centered_rank_sorted", &launch_centered_rank_sorted, py::arg("f"),
        py::arg("n"), py::arg("out"), py::arg("work"),
        py::arg("work_bytes"), py::arg("stream"));
  m.def("mlp_policy_forward", &launch_mlp_forward, py::arg("theta"),
        py::arg("x"), py::arg("batch"), py::arg("logits"),
        py::arg("stream"));
  m.def("mfma_gemm64_probe", &launch_gemm64_probe, py::arg("a"),
        py::arg("b"), py::arg("c"), py::arg("stream"));
  m.def("logits_reduce_probe", &launch_logits_reduce_probe, py::arg("p0"),
        py::arg("p1"), py::arg("out_shfl"), py::arg("out_swap"),
        py::arg("stream"));

  m.attr("NP_CONV") = 677686;
  m.attr("NP_CONV_PAD") = 677688;
  m.attr("CONV_ENVS") = 16;
  m.def("es_perturb", &launch_perturb, py::arg("theta"), py::arg("nparams"),
        py::arg("np_pad"), py::arg("sigma"), py::arg("seed"),
        py::arg("iterp"), py::arg("member_offset"), py::arg("pop"),
        py::arg("wpert"), py::arg("w3_fp8"), py::arg("w1_fp8"),
        py::arg("stream"));
  m.def("conv_env_init", &launch_conv_env_init, py::arg("seed"),
        py::arg("iterp"), py::arg("nmembers"), py::arg("state"),
        py::arg("racc"), py::arg("stream"));
  m.def("conv_noisegen", &launch_conv_noisegen, py::arg("seed"),
        py::arg("iterp"), py::arg("t"), py::arg("nenv"),
        py::arg("znoise"), py::arg("stream"));
  m.def("conv_forward", &launch_conv_forward, py::arg("wpert"),
        py::arg("w3_fp8"), py::arg("w1_fp8"), py::arg("state"),
        py::arg("gtab"), py::arg("znoise"), py::arg("act1"),
        py::arg("act2"), py::arg("act3"), py::arg("nmembers"),
        py::arg("stream"));
  m.def("conv_layer1", &launch_conv_layer1, py::arg("wpert"),
        py::arg("w1_fp8"), py::arg("state"), py::arg("gtab"),
        py::arg("znoise"), py::arg("act1"), py::arg("nmembers"),
        py::arg("stream"));
  m.def("conv_layer2", &launch_conv_layer2, py::arg("wpert"),
        py::arg("act1"), py::arg("act2"), py::arg("nmembers"),
        py::arg("stream"));
  m.def("conv_fc", &launch_conv_fc, py::arg("wpert"), py::arg("w3_fp8"),
        py::arg("act2"), py::arg("act3"), py::arg("nmembers"),
        py::arg("stream"));
  m.def("conv_head_env", &launch_conv_head_env, py::arg("wpert"),
        py::arg("act3"), py::arg("nmembers"), py::arg("env_A"),
        py::arg("env_B"), py::arg("state"), py::arg("racc"),
        py::arg("stream"));
}
