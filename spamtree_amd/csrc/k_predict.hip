// Kernel translation unit of libspamtree_hip.so: predict_points.hpp (definitions) and the launcher of st_points_predict.
#define ST_DEFS_PREDICT_POINTS 1   // this translation unit compiles the kernels of that family; the other headers give structures and prototypes
#include "predict_points.hpp"

static const char *const k_points_route_names[PP_ROUTE_COUNT] = {
  "", "k_points_mfma<128>", "k_points_mfma<256>", "k_points_generic",
};

const char *points_route_name(int code) {
  return (code >= 0 && code < PP_ROUTE_COUNT) ? k_points_route_names[code] : nullptr;
}

// Launches every kernel the point set needs on `st` (no synchronisation); *route_mask gets bit code - 1 of each one launched.
int points_launch(const PointsLaunch &L, const PointsArgs &A, const CovPar &cp, hipStream_t st, int *route_mask) {
  int mask = 0;
  if (L.ntile128 > 0) {
    PointsArgs a = A;
    a.ntiles = L.ntile128;
    const size_t lds = PP_LDS_BYTES(128);
    (void)hipFuncSetAttribute((const void *)k_points_mfma<128>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipLaunchKernelGGL((k_points_mfma<128>), dim3(L.ntile128), dim3(PP_NT), lds, st, a, cp);
    mask |= 1 << (PP_ROUTE_MFMA128 - 1);
  }
  if (L.ntile256 > 0) {
    PointsArgs a = A;
    a.tiles = A.tiles + L.ntile128;
    a.ntiles = L.ntile256;
    const size_t lds = PP_LDS_BYTES(256);
    (void)hipFuncSetAttribute((const void *)k_points_mfma<256>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipLaunchKernelGGL((k_points_mfma<256>), dim3(L.ntile256), dim3(PP_NT), lds, st, a, cp);
    mask |= 1 << (PP_ROUTE_MFMA256 - 1);
  }
  if (L.grid_generic > 0 && A.ngen > 0) {
    hipLaunchKernelGGL(k_points_generic, dim3(L.grid_generic), dim3(PP_NT), 0, st, A, cp);
    mask |= 1 << (PP_ROUTE_GENERIC - 1);
  }
  *route_mask = mask;
  return launch_rc();
}
