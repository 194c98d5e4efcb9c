// tree_layout.hpp -- the launch structures of a problem, built on the host without a HIP or RCCL call ("st_create
// in three steps").  layout_order validates the CSR topology and fixes the device block order, the ancestor lists, the
// record layout and the shard ownership (all st_shard_plan needs); layout_levels builds, from that and the device's limits,
// everything the launch sites in spamtree_hip.hip index.  The kernel headers give the structures and constants.
#pragma once
#include "st_device.hpp"
#include "factor_generic.hpp"
#include "factor_mfma.hpp"
#include "chol_blocked.hpp"
#include "factor_quad.hpp"
#include "factor_big.hpp"
#include "factor_wide.hpp"
#include "factor_lchain.hpp"
#include "sample_kernels.hpp"

struct LevelInfo {
  int first = 0, count = 0;   // into lvl_list
  int isref = 1;
  int maxP = 0, maxM = 0, maxMa = 0, maxLd = 0;
  bool big_factor = false, big_sample = false, sample_sq = false;   // sample_sq: k_sample<true> keeps S and chol(S)^-1 in LDS
  size_t lds_factor = 0, lds_sample = 0, lds_loglik = 0;
  double alg_bytes_A = 0, alg_bytes_B = 0, alg_bytes_C = 0, alg_bytes_msg = 0;
  double flops_A = 0, flops_B = 0, flops_C = 0;
  // MFMA fast path of phase A (column groups)
  bool fast = false;
  int grp_first = 0, grp_count = 0, Pm4 = 0, ldKV = 2, ldS = 2, SRm = 1, stage_dbl = 0;
  size_t lds_fast = 0;
  int ldN = 2, Mr4 = 4, Mrows = 1, av_dbl = 224, maxJ = 0;
  size_t lds_sfast = 0, lds_slean = 0;
  bool bigmfma = false;            // generic level whose phase A takes k_factor_bigmfma
  int wide_first = 0, wide_count = 0, wide_maxN = 0;   // sibling groups of this rank's run (k_factor_wide); count 0: not used
  size_t lds_wide = 0;
  int bm_ldS = 0;
  size_t lds_bigmfma = 0;
  int lchain = 0;                  // non-reference level on k_factor_lchain<lchain> (0: not used)
  bool lchain_ref = false;         // ... a REFERENCE level: k_factor_lchain, then k_factor_ref_finish
  size_t lds_ref_finish = 0;
  int rf_first = 0;                // its blocks' entries (this rank's run) in d_rfvoff / d_rfvld
  int lc_first = 0, lc_count = 0;  // its slabs (this rank's run) in d_lcslabs
  int quad_first = 0, quad_count = 0, qown_lo = 0, qown_n = 0, q_ldS = 0, q_nkx = 0;   // k_factor_quad (q_nkx = 0: not eligible)
  long long qr_off = -1;           // level on k_factor_quad with quads of this rank: its records in qrec (8-byte words) ...
  int qr_words = 0;                // ... and a record's length
  long long vl_off = -1;           // leaf quad level whose T a proposal defers: its V tiles in d_vleaf (-1: always QM_FULL)
  size_t lds_quad = 0;
  int own_lo = 0, own_n = 0, gown_lo = 0, gown_n = 0;   // this rank's run of the level's block list / group list
};

// The library's environment switches ("Runtime switches", says what each one does), read once per create.
// The defaults are the measured best.  wide, split_gram, sample_wave: 0 never, 2 on every eligible level.
struct Switches {
  int wide = 1, split_gram = 1, sample_wave = 1;
  bool lchain = true, lchain_ref = true, gram_big = true, gram_direct = true, sample_lean = true, sample_lat = true,
       leaf_seg = true, leaf_wide = true, async_top = true;
  int lchain_ref_min = 1;
  int factor_gen = 3;     // 3: k_factor_quad where a column-group level is eligible, k_factor_mfma elsewhere; 1: k_factor_mfma everywhere
  int quad_units = 0;     // k_factor_quad's units per workgroup, honoured in 1 .. quad_nu
  int quad_min = -1;      // smallest level that takes k_factor_quad (-1: 2 x CUs)
};
Switches read_switches();

// What the layout needs to know of the device and of the compiled kernels; the device step fills it before layout_levels.
struct DeviceLimits {
  static constexpr size_t QUAD_STATIC_FALLBACK = 24 * 1024, LCHAIN_STATIC_FALLBACK = 16 * 1024;   // where the attributes cannot be read
  static constexpr size_t CU_LDS = 160 * 1024;
  size_t lds_limit = 65536;      // dynamic LDS a workgroup may ask for (at most CU_LDS)
  int sm_count = 256;
  size_t quad_static = QUAD_STATIC_FALLBACK;   // static LDS of the k_factor_quad<4, 50, 13, ...> instantiations (their maximum)
  size_t lchain_static[2] = {LCHAIN_STATIC_FALLBACK, LCHAIN_STATIC_FALLBACK};   // ... of k_factor_lchain<96> / <136>
  bool lchain_no_scratch[2] = {false, false};   // ... and whether it keeps K in registers (a build that does not is never used)
};

struct TreeLayout {
  // the problem and the options that shape the layout
  long long n_all = 0, n_blocks = 0;
  int q = 1, p = 1, d = 2, n_groups = 0, n_actual_groups = 0;
  int force_generic = 0;
  bool limited = false;               // limited_tree: single parents, marginal chain factors (k_marginal_invchol)
  bool defer_leaf = false;
  Switches sw;
  size_t lds_limit = 65536;
  int sm_count = 256;
  int quad_nu = 4;                    // units per workgroup of k_factor_quad (2 per workgroup with two workgroups per CU measured slower)

  std::vector<long long> dev2model, model2dev;       // rows
  std::vector<int> blk_model2dev;                    // blocks
  std::vector<Blk> blks;                             // device block order
  std::vector<int> anc_idx, dch_idx, lvl_list, pred_list, all_obs_list;
  std::vector<Grp> grps;
  std::vector<Quad> quads;
  // quad records (QuadRec, factor_quad.hpp): what k_factor_quad's workgroups start from, per level on that kernel one record
  // per quad of this rank's run (LevelInfo::qr_off), then the prediction quads' (pred_qr_off).  The device step uploads
  // them once and drops the host copy; qrec_bytes stays
  std::vector<long long> qrec;
  size_t qrec_bytes = 0;
  long long pred_qr_off = -1;
  int pred_qr_words = 0;
  std::vector<WideGrp> wgrps;                 // sibling groups of the wide levels (k_factor_wide)
  std::vector<LcSlab> lcslabs;                // k_factor_lchain: slabs of sibling groups
  std::vector<long long> rfvoff;   // k_factor_ref_finish: per block of a reference level on the lchain route, its columns in the V scratch
  size_t vscr_need = 0;
  std::vector<long long> gdesc;               // group descriptors (GdHead layout), gd_stride words per group
  int gd_stride = 8;
  std::vector<long long> s0off;               // per block: offset of its Ri' Ri in d_s0, -1 = none
  size_t s0_total = 0;
  // multi-GPU sharding
  int rank = 0, world = 1, cut = 0;
  std::vector<int> blk_owner;                 // device block -> owning rank, -1 = replicated
  std::vector<int> own_obs_list;              // observed blocks this rank evaluates in phase C
  std::vector<int> own_grp_list, own_obs_slow; // the same set split: column groups of the fast levels / blocks of the others
  std::vector<unsigned char> rowmask, blkmask; // 1 = this rank contributes the entry to a sum-with-zeros exchange
  std::vector<int> gidx;                      // all-gather of w: device row of every slot, world x gather_cnt (-1: padding / the failure word)
  int gather_cnt = 1;
  long long top_off = 0, top_len = 0;         // message records of the cut level inside `acc`
  std::vector<std::pair<long long, long long>> top_zero;   // sub-ranges of it owned by other ranks
  std::vector<int> top_list;                  // this rank's observed blocks of the levels st_factor_begin may run ahead
  int n_toplist = 0, g_top = 0;
  int gram_direct_level = -1;                 // >= 0: that (last reference) level forms its children's Gram parts itself: k_gram_direct
  std::vector<int> twin_list;         // limited_tree: device ids of the blocks that own a chain panel
  int twin_maxM = 1;
  std::vector<LevelInfo> levels;
  LevelInfo pred_info;
  int pred_grp_first = 0, pred_grp_count = 0, pred_quad_first = 0, pred_quad_count = 0, pred_nkx = 0;   // phase P on k_factor_quad's leaf path (pred_nkx = 0: generic kernel)
  size_t pred_lds = 0;
  size_t panel_total = 0, acc_total = 0;
  long long scratch_stride = 0;               // the generic kernels' scratch: scratch_wgs slices of scratch_stride doubles (0: none)
  int scratch_wgs = 0;
  size_t vleaf_total = 0;                     // doubles of the deferred leaf levels' V tiles (their LevelInfo::vl_off)
};

inline size_t lds_loglik_bytes(int maxP, int maxM) { return ((size_t)maxP + 2 * (size_t)maxM) * 8 + 64; }

// Each returns ST_OK, or the ST_ERR_* code of the first failing check with its text in msg.
int layout_order(const st_problem *pb, const st_options *opt, TreeLayout &t, std::string &msg);
int layout_levels(const st_problem *pb, const Switches &sw, const DeviceLimits &dl, TreeLayout &t, std::string &msg);
