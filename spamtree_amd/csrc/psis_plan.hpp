// The host-only part of the Pareto-smoothing kernel's launch (psis_kernels.hpp): the tile plan, the tail length and the refusals of a
// store's shape.  Pure C++ (no HIP): tests/psis_plan_check.cpp compiles psis_plan.cpp alone.
#pragma once
#include <cstddef>
#include <string>

#include "spamtree_hip.h"

#define PSIS_NT 256              // four waves: the sort wants threads, the fit one wave per series
#define PSIS_MAX_R 8             // series per tile at most (RANK_MAX_R)
#define PSIS_TILE (64 * 1024)    // the LDS a workgroup aims for; a longer series takes what the device allows
#define PSIS_LDS_STATIC 1024     // room left for the kernel's static LDS
#define PSIS_MAX_WGS 1024        // grid cap
#define PSIS_MAX_DRAWS ST_PSIS_MAX_DRAWS
#define PSIS_MAX_TAIL 384        // min(S / 5, ceil(3 sqrt S)) at S = 16384
#define PSIS_MAX_GRID 49         // 30 + isqrt(384)

// the tail length of S finite draws: min(S / 5, m*), m* the smallest integer with m*^2 >= 9 S
int psis_tail_length(long long S);
// the dynamic LDS of a tile: R rows of Kpad sorted values and R rows of PSIS_MAX_TAIL tail values
size_t psis_lds_bytes(int R, int Kpad);
// R and Kpad of a store of K draws under a per-workgroup LDS limit; false: the sorted copy of one series does not fit
bool psis_plan(long long K, size_t lds_limit, int *R, int *Kpad);
// the workgroups of a launch over n series
long long psis_grid(long long n, int R);
// what st_rows_loo_reserve refuses of `keep`, what st_psis refuses of K: ST_OK, or the code with the text in msg
int psis_check_draws(const char *who, const char *what, long long K, std::string &msg);
// an accumulate into column `col` of a store of `keep` columns (keep == 0: no store, nothing to refuse)
int psis_check_column(const char *who, long long col, long long keep, std::string &msg);
// the store's bytes: three [keep][n] arrays of doubles
double psis_store_bytes(long long keep, long long n);
