// Kernel translation unit of libspamtree_hip.so: simulate_kernels.hpp (definitions) and the launcher of st_simulate.
#define ST_DEFS_SIMULATE 1   // this translation unit compiles the kernels of that family; the other headers give structures and prototypes
#include "simulate_kernels.hpp"

static const char *const k_sim_route_names[SIM_ROUTE_COUNT] = {
  "", "k_sim_wave<32>", "k_sim_wave<64>", "k_sim_leaf", "k_sim_generic",
};

const char *simulate_route_name(int code) {
  return (code >= 0 && code < SIM_ROUTE_COUNT) ? k_sim_route_names[code] : nullptr;
}

// a function of the tree only (never of nd), so that a draw takes the same kernels whatever batch it rides in
int simulate_route(bool isref, int maxM, bool force_generic) {
  if (force_generic) return SIM_ROUTE_GENERIC;
  if (!isref) return SIM_ROUTE_LEAF;
  if (maxM <= 32) return SIM_ROUTE_WAVE32;
  if (maxM <= 64) return SIM_ROUTE_WAVE64;
  return SIM_ROUTE_GENERIC;
}

int simulate_normals(double *out, const long long *dev2model, long long n, int nd, int nd_pad, unsigned iter0, unsigned stream,
                     unsigned long long seed, hipStream_t st) {
  const long long cnt = n * nd_pad;
  if (cnt > 0)
    hipLaunchKernelGGL(k_sim_normals, dim3((unsigned)((cnt + SIM_NT - 1) / SIM_NT)), dim3(SIM_NT), 0, st, out, dev2model, n, nd,
                       nd_pad, iter0, stream, seed);
  return launch_rc();
}

template <int ND>
static void launch_level(const SimLevel &L, const SimArgs &A0, hipStream_t st) {
  SimArgs A = A0;
  A.list = A0.list + L.first;
  A.nlist = L.count;
  A.row_lo = L.row_lo;
  A.row_hi = L.row_hi;
  const int wpg = SIM_NT / 64;
  switch (L.route) {
    case SIM_ROUTE_WAVE32:
      hipLaunchKernelGGL((k_sim_wave<32, ND>), dim3((L.count + wpg - 1) / wpg), dim3(SIM_NT), SIM_WAVE_LDS(32), st, A);
      break;
    case SIM_ROUTE_WAVE64:
      (void)hipFuncSetAttribute((const void *)k_sim_wave<64, ND>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)SIM_WAVE_LDS(64));
      hipLaunchKernelGGL((k_sim_wave<64, ND>), dim3((L.count + wpg - 1) / wpg), dim3(SIM_NT), SIM_WAVE_LDS(64), st, A);
      break;
    case SIM_ROUTE_LEAF:
      hipLaunchKernelGGL((k_sim_leaf<ND>), dim3((unsigned)((L.row_hi - L.row_lo + wpg - 1) / wpg)), dim3(SIM_NT), 0, st, A);
      break;
    default: {
      const size_t lds = SIM_GEN_LDS(L.maxM, ND);
      (void)hipFuncSetAttribute((const void *)k_sim_generic<ND>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
      hipLaunchKernelGGL((k_sim_generic<ND>), dim3(L.count), dim3(SIM_NT), lds, st, A);
    }
  }
}

int simulate_launch(const SimLevel *lv, int nlev, const SimArgs &A, int nd_pad, hipStream_t st, int *route_mask) {
  int mask = 0;
  for (int g = 0; g < nlev; ++g) {
    const SimLevel &L = lv[g];
    if (L.count == 0) continue;
    switch (nd_pad) {
      case 1: launch_level<1>(L, A, st); break;
      case 2: launch_level<2>(L, A, st); break;
      case 4: launch_level<4>(L, A, st); break;
      case 8: launch_level<8>(L, A, st); break;
      default: launch_level<16>(L, A, st);
    }
    mask |= 1 << (L.route - 1);
    if (const int e = launch_rc()) { *route_mask = mask; return e; }
  }
  *route_mask = mask;
  return 0;
}
