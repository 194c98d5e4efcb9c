// The host-only part of the mixture kernels' launches (points_mixture.hpp): how many series a workgroup of k_mix_quantile and
// k_mix_crps takes, their dynamic LDS and their grids, from the number of stored components K, the number of series n and the
// device's per-workgroup LDS limit.  Pure C++ (no HIP call): tests/mixture_plan_check.cpp compiles mixture_plan.cpp alone.
#pragma once
#include <cstddef>

#include "spamtree_hip.h"

#define MIX_NT 256                 // four waves a workgroup, both kernels
#define MIX_MAX_DRAWS ST_MIX_MAX_DRAWS
#define MIX_MAX_PROBS ST_MIX_MAX_PROBS
#define MIX_Q_MAX_R 8              // k_mix_quantile: series per workgroup at most (two per wave)
#define MIX_Q_TILE (32 * 1024)     // ... and the LDS it aims for; a longer series takes what it needs
#define MIX_C_RED 128              // k_mix_crps: bytes of cross-wave reduction beside the staged components (4 waves x 3 sums, padded)

struct MixPlan {
  int R = 0;            // series (k_mix_quantile) or scored points (k_mix_crps) per workgroup
  int G = 0;            // threads that work on one series: 64 in k_mix_quantile; 64, 128 or 256 in k_mix_crps (a function of K alone)
  size_t lds = 0;       // dynamic LDS of a workgroup in bytes
  long long grid = 0;   // workgroups: ceil(n / R)
};

// k_mix_quantile: a wave per series, R = min(MIX_Q_MAX_R, max(4, MIX_Q_TILE / (16 K))) series staged as (m, sd) pairs -- but never more
// rows than the LDS limit holds.  false: K outside 1 .. MIX_MAX_DRAWS, n < 1, or one series does not fit the limit.
bool mix_quantile_plan(long long K, long long n, size_t lds_limit, MixPlan *P);
// k_mix_crps: G = 64 threads a point up to K = 64, 128 up to K = 128, else all 256; R = MIX_NT / G points a workgroup, each staged
// as K (mu, sigma2) pairs, and MIX_C_RED bytes for the cross-wave sums.  false as above.
bool mix_crps_plan(long long K, long long n, size_t lds_limit, MixPlan *P);
// the pairs s < t one scored point costs: K (K - 1) / 2
double mix_crps_pairs(long long K);
// the store's bytes per saved draw: 16 B per point (24 B with X), 8 q for tau2, 16 B per functional
double mix_store_bytes(long long n, bool has_X, int q, long long n_fun);
