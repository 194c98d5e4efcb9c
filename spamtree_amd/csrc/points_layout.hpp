// points_layout.hpp -- the launch structures of a set of new points (st_points_set, st_points_set_joint), built on the host
// without a HIP call ("st_points_set in two steps"): the caller's arrays validated, every point's conditioning chain,
// the chains' kernel classes, the sorted order and its tiles and, for a joint set, the groups and their packing into the
// 16-column slots of k_points_joint_mfma.  The device step in st_points.hip uploads the lists and keeps the counts.
#pragma once
#include "tree_layout.hpp"
#include "predict_joint.hpp"
#include "points_fun.hpp"

// what the launch sites read after st_points_set has returned
struct PointsCounts {
  int ntile128 = 0, ntile256 = 0, grid_generic = 0, n_chains = 0;   // tiles [0, ntile128) take <128>, the next ntile256 <256>
  long long scratch_stride = 1;                // doubles per scratch column of the generic routes: the longest generic chain, padded to 32
  double alg_bytes = 0.0, flops = 0.0;
  // a joint set
  long long n_joint = 0, cov_total = 0;
  int jtile128 = 0, jtile256 = 0, jgrid_generic = 0;
  double j_alg_bytes = 0.0, j_flops = 0.0;
};

struct PointsLayout : PointsCounts {
  std::vector<PtChain> chains;                 // by their last block's device id (an empty conditioning set first)
  std::vector<int> chain_blk;
  std::vector<long long> order;                // sorted point -> caller index: 128-row chains, 256-row chains, generic; by chain, by caller index
  std::vector<int> pt_chain;                   // per sorted point
  std::vector<PtTile> tiles;                   // of the non-generic part of the sorted list
  std::vector<int> gen;                        // the sorted points of generic chains
  // a joint set (joint_id given): groups in order of first appearance, members in the caller's order
  std::vector<int64_t> j_off, j_mptr, j_mem;   // packed block offsets (n_joint + 1), member list pointers (n_joint + 1), members
  std::vector<int> pt_grp, pt_a;               // per point, caller order: its group and member index
  std::vector<PtJoint> groups;
  std::vector<PtTile> jtiles;                  // np: slots in use
  std::vector<PtCol> jcols;                    // PP_NCOL per tile (one dummy entry without a tile)
  std::vector<int> jgen;                       // the groups of generic chains
};

// Returns ST_OK, or the ST_ERR_* code of the first failing check with its text in msg.  joint_id NULL: st_points_set.
int points_layout(const TreeLayout &t, int64_t n_new, const double *coords, const int64_t *mv, const int64_t *anchor,
                  const int64_t *joint_id, PointsLayout &out, std::string &msg);

// ---- linear functionals of the point set (st_points_functionals_set; points_fun.hpp has the term lists and the kernels) ----
// what functionals_layout reads of the current point set: its size and, of a joint set, the groups
struct FunFacts {
  long long n = 0;                             // points
  bool joint = false;
  const int64_t *j_off = nullptr, *j_mptr = nullptr;   // n_joint + 1 each (PointsLayout)
  const int *pt_grp = nullptr, *pt_a = nullptr;        // per point, caller order
};

struct FunLayout {
  long long n_fun = 0, nnz = 0, n_var_terms = 0;
  std::vector<FunTerm> lin, var;               // the linear and the variance list, functional after functional
  std::vector<FunChunk> lin_chunks, var_chunks;   // each list cut into chunks of <= FUN_CHUNK terms of one functional
  std::vector<long long> lin_cptr, var_cptr;   // n_fun + 1 each: functional f owns chunks [cptr[f], cptr[f + 1]) of its list
  double alg_bytes(bool has_yhat) const {      // per saved iteration: terms, gathered values, chunk sums out and in, k_fun_finish
    const double nc = (double)(lin_chunks.size() + var_chunks.size());
    return 16.0 * (double)(nnz + n_var_terms) + 8.0 * ((has_yhat ? 3.0 : 2.0) * (double)nnz + (double)n_var_terms) + 64.0 * nc +
           (double)n_fun * (2.0 * PA_NACC * 8.0 + 4 * 8.0 + 2 * 8.0 + 4 * 8.0);
  }
};

// CSR functionals on the point set `p`: the argument checks of st_points_functionals_set and the two chunked term lists.
// Returns ST_OK, or ST_ERR_USAGE with the functional and entry named in msg.
int functionals_layout(const FunFacts &p, int64_t n_fun, const int64_t *ptr, const int64_t *idx, const double *wt, FunLayout &out,
                       std::string &msg);
