// lgo_layout.hpp -- the groups of the leave-group-out criteria (st_rows_loo_groups_*, lgo_kernels.hpp) and what the pair part of
// the upward sweep indexes, built on the host from a TreeLayout, its LooLayout and a label per row without a HIP call.
//
//   groups    the rows with one non-negative label that lie in a block of the density; labelled rows of prediction blocks are
//             ignored.  Groups are numbered by ascending label, a group's members stand in ascending model row: grp_ptr (CSR),
//             mem_row (device rows), mem_model (model rows), label.  1 .. LGO_MAX_MEMBERS members, at least one with an observed y.
//   pr_ptr,   per device block u (CSR): its pair list, the column pairs (a, b), a < b < P + m, of [chain ; own] whose rows share a
//   pr_a,     group, sorted by (b, a).  Left out are the structural zeros a block can see: two own rows of a non-reference block.
//   pr_b,     (Two rows whose blocks lie on no common root-to-leaf path never meet in one column list.)  A direct child's columns
//   pr_fin    are its parent's followed by its own, so the child's pairs with b < P_child are exactly its parent's pairs in the
//             same order: the p part of S_child lines up with S_parent's by prefix, as the d and c parts do.  pr_fin: the slot
//             of the finished value in the per-pair array where the pair is complete here -- at the block that holds its deeper
//             member, b >= P -- and -1 elsewhere.
//   voff,     S_u grows by its n_pairs_u doubles, the p part at [2 (P + m), 2 (P + m) + n_pairs_u); a block without pairs grows
//   arena     by nothing.  These replace LooLayout's while groups are set.
//   gp_ptr,   per group (CSR, g (g - 1) / 2 entries): for the members i < j, at j (j - 1) / 2 + i, the slot of Q_ij in the per-pair
//   gp_idx    array, or -1 for a structural zero.
#pragma once
#include "loo_layout.hpp"

#define LGO_MAX_MEMBERS 16   // = ST_ROWS_LGO_MAX_MEMBERS

struct LgoLayout {
  long long n_groups = 0, n_members = 0, n_pairs = 0;   // n_pairs: the slots of the per-pair array (finished pairs)
  long long n_pair_slots = 0;                           // the pair slots of all blocks' S_u
  std::vector<long long> label;
  std::vector<int> grp_ptr;
  std::vector<long long> mem_row, mem_model;
  std::vector<int> pr_ptr, pr_a, pr_b, pr_fin;
  std::vector<long long> voff;
  long long arena = 0;
  std::vector<int> gp_ptr, gp_idx;
  int max_block_pairs = 0;
  double alg_bytes = 0, flops = 0;   // what the pair part and the group kernel add to one st_rows_loo_accumulate, from shapes
};

// labels: n_all values in model row order, negative = in no group.  obs: n_all flags in device row order (an observed y).
// ST_OK, or the ST_ERR_* code of the first failing check with its text in msg: more than LGO_MAX_MEMBERS members
// (ST_ERR_UNSUPPORTED, with both numbers), a group without an observed member (ST_ERR_USAGE), member pairs, pair slots or entries of
// the groups' g x g matrices beyond what 32-bit indices reach (ST_ERR_UNSUPPORTED, with both numbers).
int lgo_layout(const TreeLayout &t, const LooLayout &lo, const long long *labels, const unsigned char *obs, LgoLayout &o, std::string &msg);
