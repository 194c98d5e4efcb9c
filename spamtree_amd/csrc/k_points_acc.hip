// Kernel translation unit of libspamtree_hip.so: the per-point predictive summaries of st_points_accumulate
// (PointsAccArgs in predict_points.hpp).  Kept apart from k_predict.hip, whose launches are the k_points_* routes.
#include "predict_points.hpp"

// One thread per point: reads the four outputs of this iteration (32 B) and the five accumulators (40 B), writes the five
// accumulators back (40 B) and, with a reservation, the draw and yhat into their rows of the [keep][n] stores (16 B).
// Each point's statistics depend on its own values in saved order only: deterministic and independent of the point order.
__global__ __launch_bounds__(NT) void k_points_acc(PointsAccArgs A) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= A.n) return;
  const long long n = A.n;
  double *acc = A.acc;
  const double x = A.mean[i], w = A.w[i];
  const double m0 = acc[PA_MEAN * n + i];
  const double d = x - m0;
  const double m1 = m0 + d / A.count;
  acc[PA_MEAN * n + i] = m1;
  acc[PA_M2 * n + i] += d * (x - m1);
  acc[PA_VAR * n + i] += A.var[i];
  acc[PA_W * n + i] += w;
  if (A.keep_w) A.keep_w[i] = w;
  if (A.yhat) {
    const double y = A.yhat[i];
    acc[PA_YHAT * n + i] += y;
    if (A.keep_yhat) A.keep_yhat[i] = y;
  }
}

int points_acc_launch(const PointsAccArgs &A, hipStream_t st) {
  if (A.n <= 0) return 0;
  hipLaunchKernelGGL(k_points_acc, dim3((unsigned)((A.n + NT - 1) / NT)), dim3(NT), 0, st, A);
  return launch_rc();
}
