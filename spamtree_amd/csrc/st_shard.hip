// st_shard.hip -- one problem shared by several ranks: everything that needs a communicator (st_comm_*, the native RCCL exchanges
// and the exchange branch of each entry point of the iteration, shard_*) or serves an exchange the caller runs (st_mg_*).  The
// state is the handle's Exchange (st_handle.hpp).  The phases themselves are launched by st_factor.hip and st_sweep.hip through
// their *_local entry points.
#include "st_handle.hpp"
#include "misc_kernels.hpp"

#define NCHK(h, call)                                                                                        \
  do {                                                                                                        \
    ncclResult_t r_ = (call);                                                                                 \
    if (r_ != ncclSuccess) { (h)->err = std::string(#call) + ": " + ncclGetErrorString(r_); return ST_ERR_HIP; } \
  } while (0)

bool uses_exchange(st_handle h) { return h->world > 1 || h->xch.comm; }   // an attached communicator selects the exchange protocol even with one rank (tests)
// ... without a communicator: the refusal; `alternatives`: the entry points that leave the exchanges to the caller
static int refuse_without_comm(st_handle h, const char *alternatives) {
  h->err = std::string("world > 1: call st_comm_init first, or use ") + alternatives;
  return ST_ERR_USAGE;
}

extern "C" int st_comm_unique_id(void *out, int32_t cap) {
  if (!out || cap < (int32_t)sizeof(ncclUniqueId)) return ST_ERR_USAGE;
  ncclUniqueId id;
  if (ncclGetUniqueId(&id) != ncclSuccess) return ST_ERR_HIP;
  std::memcpy(out, &id, sizeof(id));
  return (int)sizeof(id);
}
extern "C" int st_comm_init(st_handle h, const void *unique_id) {
  if (!h || !unique_id) return ST_ERR_USAGE;
  HCHK(h, hipSetDevice(h->device));
  ncclUniqueId id;
  std::memcpy(&id, unique_id, sizeof(id));
  NCHK(h, ncclCommInitRank(&h->xch.comm, h->world, id, h->rank));
  return ST_OK;
}
void comm_free(st_handle_s *h) {
  if (h->xch.comm) (void)ncclCommDestroy(h->xch.comm);
}

// sum-with-zeros exchange buffers: every entry is contributed by exactly one rank (replicated blocks by rank 0), so
// an all-reduce(sum) reproduces the single-GPU arrays bit for bit, for any number of ranks and any reduction order
// all-gather form of the exchange of w: a rank's slice of the gather buffer = its owned rows + its failure word
extern "C" int st_mg_pack_comps(st_handle h, int slot, void **dev_ptr, int64_t *len) {
  if (!h || slot < 0 || slot > 1) return ST_ERR_USAGE;
  HCHK(h, hipSetDevice(h->device));
  { const int rc0 = settle_top(h); if (rc0) return rc0; }
  const int phys = h->slot_map[slot], nb = (int)h->n_blocks;
  {
    ProfScope ps(h, 3);
    hipLaunchKernelGGL(k_pack_comps, dim3((std::max(nb, h->world) + NT - 1) / NT), dim3(NT), 0, h->stream, h->d_logdet[phys].p,
                       h->d_loglik[phys].p, h->xch.d_blkmask.p, nb, h->d_err.p, h->rank, h->world, h->xch.d_comm.p);
  }
  HCHK(h, hipGetLastError());
  if (dev_ptr) *dev_ptr = h->xch.d_comm.p;
  if (len) *len = 2 * (int64_t)nb + h->world;
  return ST_OK;
}

// The sums of the exchanged components (st_mg_pack_comps + all-reduce) on their way to dst like enqueue_result's, with the ranks' failure words behind them
static int enqueue_comm_result(st_handle h, Landing *dst, double *rank_words) {
  const int nb = (int)h->n_blocks;
  if (const int rc = enqueue_result(h, h->xch.d_comm.p, h->xch.d_comm.p + nb, nb, dst)) return rc;
  HCHK(h, hipMemcpyAsync(rank_words, h->xch.d_comm.p + 2 * (size_t)nb, h->world * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  return ST_OK;
}

// after the exchange of the packed components: deterministic sum + failure code agreed by all ranks
extern "C" int st_mg_finish(st_handle h, double *loglik) {
  if (!h) return ST_ERR_USAGE;
  HCHK(h, hipSetDevice(h->device));
  Landing res;
  double errc[ST_MAX_RANKS];
  if (const int rc = enqueue_comm_result(h, &res, errc)) return rc;
  HCHK(h, hipStreamSynchronize(h->stream));
  if (const int code = rank_failure(errc, h->world)) return code;
  return landing_code(res, loglik);
}

// pack -> RCCL all-reduce(sum) on the launch stream -> deterministic finish (native path of the multi-GPU protocol)
static int exchange_comps_and_finish(st_handle h, int slot, double *loglik) {
  void *ptr = nullptr;
  int64_t len = 0;
  int rc = st_mg_pack_comps(h, slot, &ptr, &len);
  if (rc) return rc;
  {
    ProfScope ps(h, 7);
    NCHK(h, ncclAllReduce(ptr, ptr, (size_t)len, ncclDouble, ncclSum, h->xch.comm, h->stream));
  }
  return st_mg_finish(h, loglik);
}

extern "C" int st_mg_top_region(st_handle h, void **dev_ptr, int64_t *len) {
  if (!h) return ST_ERR_USAGE;
  if (dev_ptr) *dev_ptr = h->d_acc.p + h->top_off;
  if (len) *len = h->top_len;
  return ST_OK;
}
extern "C" int st_mg_pack_w(st_handle h, void **dev_ptr, int64_t *len) {
  if (!h) return ST_ERR_USAGE;
  HCHK(h, hipSetDevice(h->device));
  const long long nn = std::max<long long>(h->n_all, h->world);
  hipLaunchKernelGGL(k_pack_w, dim3((unsigned)((nn + NT - 1) / NT)), dim3(NT), 0, h->stream, h->d_w.p, h->xch.d_rowmask.p, h->n_all, h->d_err.p,
                     h->rank, h->world, h->d_tmp_n.p);
  HCHK(h, hipGetLastError());
  if (dev_ptr) *dev_ptr = h->d_tmp_n.p;
  if (len) *len = h->n_all + h->world;
  return ST_OK;
}
extern "C" int st_mg_unpack_w(st_handle h) {
  if (!h) return ST_ERR_USAGE;
  invalidate_stats(h);
  HCHK(h, hipSetDevice(h->device));
  double errw[ST_MAX_RANKS];
  HCHK(h, hipMemcpyAsync(h->d_w.p, h->d_tmp_n.p, (size_t)h->n_all * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
  HCHK(h, hipMemcpyAsync(errw, h->d_tmp_n.p + h->n_all, h->world * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HCHK(h, hipStreamSynchronize(h->stream));
  return rank_failure(errw, h->world);
}

// all-gather form (half the traffic of the all-reduce of n doubles): pack -> all-gather(recv, count per rank) -> unpack
extern "C" int st_mg_gather_w_pack(st_handle h, void **send_ptr, void **recv_ptr, int64_t *count_per_rank) {
  if (!h) return ST_ERR_USAGE;
  HCHK(h, hipSetDevice(h->device));
  const int cnt = h->gather_cnt;
  double *mine = h->xch.d_gather.p + (size_t)h->rank * cnt;
  hipLaunchKernelGGL(k_gather_pack, dim3((cnt + NT - 1) / NT), dim3(NT), 0, h->stream, h->d_w.p, h->xch.d_gidx.p + (size_t)h->rank * cnt, cnt,
                     h->d_err.p, mine);
  HCHK(h, hipGetLastError());
  if (send_ptr) *send_ptr = mine;
  if (recv_ptr) *recv_ptr = h->xch.d_gather.p;
  if (count_per_rank) *count_per_rank = cnt;
  return ST_OK;
}
static int gather_w_scatter(st_handle h) {   // launches only: rows into w, failure words into d_gerr
  const long long total = (long long)h->world * h->gather_cnt;
  hipLaunchKernelGGL(k_gather_unpack, dim3((unsigned)((total + NT - 1) / NT)), dim3(NT), 0, h->stream, h->xch.d_gather.p, h->xch.d_gidx.p, h->gather_cnt,
                     total, h->d_w.p, h->xch.d_gerr.p);
  HCHK(h, hipGetLastError());
  return ST_OK;
}
extern "C" int st_mg_gather_w_unpack(st_handle h) {
  if (!h) return ST_ERR_USAGE;
  invalidate_stats(h);
  HCHK(h, hipSetDevice(h->device));
  int rc = gather_w_scatter(h);
  if (rc) return rc;
  double errw[ST_MAX_RANKS];
  HCHK(h, hipMemcpyAsync(errw, h->xch.d_gerr.p, h->world * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HCHK(h, hipStreamSynchronize(h->stream));
  return rank_failure(errw, h->world);
}

// The sweep's exchange (communicator attached) up to the gather-pack: this rank's subtrees, all-reduce of the cut level's message
// records, the replicated top levels, then the rank's own rows of w and its failure word packed for the all-gather.
static int sweep_exchange(st_handle h, const double *z, uint64_t seed, uint32_t iter, void **send, void **recv, int64_t *count) {
  int rc = st_sample_w_local(h, z, seed, iter);
  if (rc) return rc;
  if (h->top_len > 0) {
    ProfScope ps(h, 7);
    NCHK(h, ncclAllReduce(h->d_acc.p + h->top_off, h->d_acc.p + h->top_off, (size_t)h->top_len, ncclDouble, ncclSum, h->xch.comm, h->stream));
  }
  rc = st_sample_w_top(h);
  if (rc) return rc;
  return st_mg_gather_w_pack(h, send, recv, count);
}

// ---- the exchange branch of each entry point of the iteration (st_factor.hip, st_sweep.hip: `if (uses_exchange(h)) return shard_...`)
int shard_factor(st_handle h, int slot, const double *theta, int ntheta, double *loglik) {
  if (!h->xch.comm) return refuse_without_comm(h, "st_factor_local / st_mg_pack_comps / (all-reduce) / st_mg_finish");
  int rc = st_factor_local(h, slot, theta, ntheta);
  if (rc) return rc;
  return exchange_comps_and_finish(h, slot, loglik);
}
// with a communicator attached st_factor_enqueue enqueues nothing and st_factor_finish does all of st_factor
int shard_factor_enqueue(st_handle h, int slot, const double *theta, int ntheta) {
  h->factor_open = true; h->factor_open_slot = slot; h->top_theta_open.assign(theta, theta + ntheta);
  return ST_OK;
}
int shard_factor_finish(st_handle h, double *loglik) {
  if (!h->xch.comm) return refuse_without_comm(h, "st_factor_local / st_mg_pack_comps / (all-reduce) / st_mg_finish");
  int rc = st_factor_local(h, h->factor_open_slot, h->top_theta_open.data(), (int)h->top_theta_open.size());
  if (rc) return rc;
  return exchange_comps_and_finish(h, h->factor_open_slot, loglik);
}
int shard_sample_w(st_handle h, const double *z, uint64_t seed, uint32_t iter) {
  if (!h->xch.comm) return refuse_without_comm(h, "st_sample_w_local / st_mg_top_region / st_sample_w_top / st_mg_pack_w / st_mg_unpack_w");
  void *snd = nullptr, *rcv = nullptr;
  int64_t cnt = 0;
  int rc = sweep_exchange(h, z, seed, iter, &snd, &rcv, &cnt);
  if (rc) return rc;
  {
    ProfScope ps(h, 7);
    NCHK(h, ncclAllGather(snd, rcv, (size_t)cnt, ncclDouble, h->xch.comm, h->stream));
  }
  return st_mg_gather_w_unpack(h);
}
int shard_loglik_w(st_handle h, int slot, double *loglik) {
  if (!h->xch.comm) return refuse_without_comm(h, "st_loglik_local / st_mg_pack_comps / (all-reduce) / st_mg_finish");
  int rc = st_loglik_local(h, slot);
  if (rc) return rc;
  return exchange_comps_and_finish(h, slot, loglik);
}
int shard_sample_w_loglik(st_handle h, const double *z, uint64_t seed, uint32_t iter, int slot, double *loglik) {
  if (!h->xch.comm) {
    int rc = st_sample_w(h, z, seed, iter);   // reports the missing communicator
    if (rc) return rc;
    return st_loglik_w(h, slot, loglik);
  }
  // Fused exchange: the log-density of a rank's own blocks needs w of its own subtrees and of the replicated top only,
  // both current BEFORE the other ranks' rows arrive -- so phase C runs ahead of the exchange of w, and w and the
  // log-density components travel in ONE grouped RCCL call, followed by ONE host synchronisation.
  void *pw = nullptr, *pr = nullptr, *pc = nullptr;
  int64_t lw = 0, lc = 0;
  int rc = sweep_exchange(h, z, seed, iter, &pw, &pr, &lw);   // own rows of w + this rank's failure word of the sweep
  if (rc) return rc;
  rc = st_loglik_local(h, slot);          // resets the failure word after the pack above (stream order)
  if (rc) return rc;
  rc = st_mg_pack_comps(h, slot, &pc, &lc);
  if (rc) return rc;
  {
    ProfScope ps(h, 7);
    NCHK(h, ncclGroupStart());
    NCHK(h, ncclAllGather(pw, pr, (size_t)lw, ncclDouble, h->xch.comm, h->stream));
    NCHK(h, ncclAllReduce(pc, pc, (size_t)lc, ncclDouble, ncclSum, h->xch.comm, h->stream));
    NCHK(h, ncclGroupEnd());
  }
  rc = gather_w_scatter(h);
  if (rc) return rc;
  invalidate_stats(h);
  Landing res;
  double errw[ST_MAX_RANKS], errc[ST_MAX_RANKS];
  rc = enqueue_comm_result(h, &res, errc);
  if (rc) return rc;
  HCHK(h, hipMemcpyAsync(errw, h->xch.d_gerr.p, h->world * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HCHK(h, hipStreamSynchronize(h->stream));
  if (const int code = rank_failure(errw, h->world)) return code;   // the sweep's words first, then the components'
  if (const int code = rank_failure(errc, h->world)) return code;
  return landing_code(res, loglik);
}
// _begin simply runs the synchronous protocol and _end hands its result over
int shard_sample_w_loglik_begin(st_handle h, const double *z, uint64_t seed, uint32_t iter, int slot) {
  h->c_ll = 0.0;
  h->c_rc = st_sample_w_loglik(h, z, seed, iter, slot, &h->c_ll);
  if (h->c_rc < 0) return h->c_rc;   // a HIP / RCCL / usage error: nothing is pending, the caller must not call _end
  h->c_pending = true;
  return ST_OK;
}
