// loo_layout.hpp -- the launch structures of st_rows_loo_* (loo_kernels.hpp), built on the host from a TreeLayout without a HIP
// call.  The blocks of the density are the blocks with observed rows (TreeLayout::lvl_list); prediction blocks are left out.
//
//   levels    the levels of the tree from the deepest to the root; a level's blocks stand in `list` in ascending device block id.
//   voff      per device block: where its upward vector S_u starts in one arena of doubles (-1: a block outside the density).
//             S_u has 2 (P + m) doubles: the `d` part (column sums of squares) at [0, P + m), the `c` part at [P + m, 2 (P + m)),
//             over the columns [rows of the chain of u ; rows of u].  Every block has a vector of its own (sibling leaf blocks
//             share none), so a parent adds its children one after another in list order.
//   ch_ptr,   per device block (CSR): its direct children of the density, ascending device block id.  A direct child d of u has
//   ch_idx    chain(d) = chain(u) + u, so P_d = P_u + m_u and S_d's first P_d entries of either part line up with S_u.
#pragma once
#include "tree_layout.hpp"

struct LooLevel {
  int first = 0, count = 0;   // into LooLayout::list
  int level = 0;              // the tree's level (TreeLayout::levels)
  int isref = 1;
  int maxLen = 0, maxM = 0;   // the largest P + m and m of the level
};

struct LooLayout {
  std::vector<int> list;
  std::vector<LooLevel> levels;
  std::vector<long long> voff;
  std::vector<int> ch_ptr, ch_idx;
  long long arena = 0;            // doubles
  double alg_bytes = 0, flops = 0;   // of one st_rows_loo_accumulate, from shapes (st_rows_loo_info)
};

// ST_OK, or the ST_ERR_* code of the first failing check with its text in msg.  A limited tree or a sharded one is refused
// (ST_ERR_UNSUPPORTED).
int loo_layout(const TreeLayout &t, LooLayout &o, std::string &msg);
