// st_protocol.hpp -- the pure parts of the iteration's read-back protocol: where the small device-to-host results land and how a
// failure word is decoded.  No HIP call and no HIP header: tests/protocol_check.cpp compiles it on its own.
#pragma once
#include <climits>
#include <cstddef>

// most ranks one problem is sharded over: the refusal of layout_order and the bound of the host arrays of per-rank failure words
constexpr int ST_MAX_RANKS = 64;
// most statistics (p q + q doubles) that follow their reduction to pinned memory on the second stream (stats_begin); more are
// fetched by a copy on the main stream when they are asked for
constexpr int ST_PIN_STATS = 40;

// One read-back: the two sums of a slot's component arrays and the failure word (INT_MAX: none; else level * 16 + code).
struct Landing {
  double sums[2] = {0.0, 0.0};
  int err[2] = {INT_MAX, 0};
};

// The handle's pinned host memory (one hipHostMalloc): every request that may be in flight at the same time has its own member.
struct PinnedArea {
  Landing sweep;                // st_sample_w_loglik on one GPU
  Landing deferred;             // st_sample_w_loglik_begin / _end
  Landing factor;               // st_factor_enqueue / st_factor_finish
  double stats[ST_PIN_STATS];   // stats_begin / fetch_stats
};

// The reference's code of a read-back (`word & 15`: 1 / 2 / 3 of phase A, 10 / 11 of the sweep; deeper levels hold unspecified
// values, Q5), or 0 with loglik_w = logdetCi + sum(loglik_w_comps) stored (spamtree_model.cpp:987-988, :815-816; the sums are
// meaningless after a failure)
inline int landing_code(const Landing &L, double *loglik) {
  if (L.err[0] != INT_MAX) return L.err[0] & 15;
  if (loglik) *loglik = L.sums[0] + L.sums[1];
  return 0;
}

// The ranks' failure words after an exchange (doubles; 0: none): the code of the smallest positive one -- the shallowest failing
// level of any rank -- or 0.
inline int rank_failure(const double *words, int world) {
  int best = INT_MAX;
  for (int r = 0; r < world; ++r)
    if (words[r] > 0.5 && (int)words[r] < best) best = (int)words[r];
  return best == INT_MAX ? 0 : (best & 15);
}
