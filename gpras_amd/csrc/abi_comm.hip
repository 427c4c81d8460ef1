// libgprx C ABI, the one collective of the path (gprx_comm_*): RCCL over xGMI.
#include "abi_common.h"

#include <cstring>
#include <string>

#include "comm.h"

using namespace gprx;

struct gprx_comm_ctx {
  int device = 0, rank = 0, world = 1;
  ncclComm_t comm = nullptr;
  hipStream_t stream = nullptr;
  Buf scratch;  // device staging of the host-buffer entry points
  std::string err;
};

extern "C" {

// ---- the one collective of the path: RCCL over xGMI -----------------------------------------
#define COMMNCCL(c, expr)                                                                                              \
  do {                                                                                                                 \
    ncclResult_t r_ = (expr);                                                                                          \
    if (r_ != ncclSuccess) return fail(c, GPRX_ERCCL, std::string(#expr) + ": " + rccl().GetErrorString(r_));         \
  } while (0)

// RCCL is loaded only after this process has initialised HIP and seen its devices: loaded first (measured on the MI355X
// box: ncclGetUniqueId before any HIP call) it left the process with "no ROCm-capable device is detected".
static int comm_runtime_ready() {
  int count = 0;
  HIPCHK(nullptr, hipInit(0));
  HIPCHK(nullptr, hipGetDeviceCount(&count));
  if (count <= 0) return fail(nullptr, GPRX_EHIP, "no device visible to this process");
  HIPCHK(nullptr, hipFree(nullptr));  // forces the runtime (context of the current device) into existence
  if (!rccl().load()) return fail(nullptr, GPRX_ERCCL, rccl().error);
  return GPRX_OK;
}

int gprx_comm_runtime_check(int device) {
  return guarded(nullptr, [&]() -> int { HIPCHK(nullptr, hipSetDevice(device)); return comm_runtime_ready(); });
}

int gprx_comm_unique_id(unsigned char* id128) {
  return guarded(nullptr, [&]() -> int {
    if (!id128) return fail(nullptr, GPRX_EINVAL, "null argument");
    int rc0;
    if ((rc0 = comm_runtime_ready())) return rc0;
    ncclUniqueId id;
    COMMNCCL(nullptr, rccl().GetUniqueId(&id));
    static_assert(sizeof(id) == GPRX_UNIQUE_ID_BYTES, "ncclUniqueId size");
    std::memcpy(id128, &id, sizeof(id));
    return GPRX_OK;
  });
}

int gprx_comm_init(int device, int rank, int world, const unsigned char* id128, gprx_comm* out) {
  if (!out) return fail(nullptr, GPRX_EINVAL, "out is null");
  *out = nullptr;
  if (!id128 || world <= 0 || rank < 0 || rank >= world) return fail(nullptr, GPRX_EINVAL, "bad rank / world / id");
  gprx_comm c = nullptr;
  const int rc = guarded(nullptr, [&]() -> int {
    HIPCHK(nullptr, hipSetDevice(device));
    int rc;
    if ((rc = comm_runtime_ready())) return rc;
    c = new gprx_comm_ctx();
    c->rank = rank;
    c->world = world;
    if ((rc = open_handle(c, device))) return rc;
    ncclUniqueId id;
    std::memcpy(&id, id128, sizeof(id));
    const ncclResult_t r = rccl().CommInitRank(&c->comm, world, id, rank);  // collective: every rank of the job calls it
    return r == ncclSuccess ? GPRX_OK : fail(nullptr, GPRX_ERCCL, std::string("ncclCommInitRank: ") + rccl().GetErrorString(r));
  });
  if (rc) gprx_comm_destroy(c);
  else *out = c;
  return rc;
}

int gprx_comm_destroy(gprx_comm c) {
  if (!c) return GPRX_OK;
  hipSetDevice(c->device);
  if (c->stream) hipStreamSynchronize(c->stream);
  if (c->comm) rccl().CommDestroy(c->comm);
  if (c->scratch.p) hipFree(c->scratch.p);
  if (c->stream) hipStreamDestroy(c->stream);
  delete c;
  return GPRX_OK;
}

const char* gprx_comm_last_error(gprx_comm c) { return c ? c->err.c_str() : last_error().c_str(); }

int gprx_comm_rank(gprx_comm c, int* rank, int* world) {
  return guarded(c, [&]() -> int {
    if (!c || !rank || !world) return fail(c, GPRX_EINVAL, "null argument");
    *rank = c->rank;
    *world = c->world;
    // what RCCL itself reports for this communicator (ncclCommUserRank / ncclCommCount), so that "did RCCL see N ranks" does not rest
    // on the numbers the caller passed to gprx_comm_init
    if (rccl().CommUserRank) COMMNCCL(c, rccl().CommUserRank(c->comm, rank));
    if (rccl().CommCount) COMMNCCL(c, rccl().CommCount(c->comm, world));
    return GPRX_OK;
  });
}

int gprx_comm_synchronize(gprx_comm c) {
  if (!c) return fail(c, GPRX_EINVAL, "null communicator");
  return guarded(c, [&]() -> int { HIPCHK(c, hipSetDevice(c->device)); HIPCHK(c, hipStreamSynchronize(c->stream)); return GPRX_OK; });
}

int gprx_comm_all_gather(gprx_comm c, const double* send_dev, double* recv_dev, int64_t count) {
  return guarded(c, [&]() -> int {
    if (!c || count < 0 || (count > 0 && (!send_dev || !recv_dev))) return fail(c, GPRX_EINVAL, "null argument");
    if (count == 0) return GPRX_OK;
    HIPCHK(c, hipSetDevice(c->device));
    COMMNCCL(c, rccl().AllGather(send_dev, recv_dev, (size_t)count, ncclDouble, c->comm, c->stream));
    return GPRX_OK;
  });
}

int gprx_comm_gather(gprx_comm c, const double* send_dev, double* recv_dev, int64_t count, int root) {
  return guarded(c, [&]() -> int {
    if (!c || count < 0 || root < 0 || root >= c->world || (count > 0 && !send_dev)) return fail(c, GPRX_EINVAL, "bad argument");
    if (c->rank == root && count > 0 && !recv_dev) return fail(c, GPRX_EINVAL, "recv_dev is null on the root");
    if (count == 0) return GPRX_OK;
    HIPCHK(c, hipSetDevice(c->device));
    // one group: the root posts world - 1 receives (its own block is a device copy), every other rank one send; inside a
    // node all inbound xGMI links of the root are busy at once
    COMMNCCL(c, rccl().GroupStart());
    ncclResult_t r = ncclSuccess;
    if (c->rank == root) {
      for (int p = 0; p < c->world && r == ncclSuccess; ++p)
        if (p != root) r = rccl().Recv(recv_dev + (int64_t)p * count, (size_t)count, ncclDouble, p, c->comm, c->stream);
    } else {
      r = rccl().Send(send_dev, (size_t)count, ncclDouble, root, c->comm, c->stream);
    }
    const ncclResult_t r2 = rccl().GroupEnd();
    COMMNCCL(c, r);
    COMMNCCL(c, r2);
    if (c->rank == root && recv_dev + (int64_t)root * count != send_dev)
      HIPCHK(c, hipMemcpyAsync(recv_dev + (int64_t)root * count, send_dev, sizeof(double) * count, hipMemcpyDeviceToDevice, c->stream));
    return GPRX_OK;
  });
}

int gprx_comm_all_reduce_max(gprx_comm c, double* buf_dev, int64_t count) {
  return guarded(c, [&]() -> int {
    if (!c || count < 0 || (count > 0 && !buf_dev)) return fail(c, GPRX_EINVAL, "null argument");
    if (count == 0) return GPRX_OK;
    HIPCHK(c, hipSetDevice(c->device));
    COMMNCCL(c, rccl().AllReduce(buf_dev, buf_dev, (size_t)count, ncclDouble, ncclMax, c->comm, c->stream));
    return GPRX_OK;
  });
}

int gprx_comm_all_gather_host(gprx_comm c, const double* send, double* recv, int64_t count) {
  return guarded(c, [&]() -> int {
    if (!c || count < 0 || (count > 0 && (!send || !recv))) return fail(c, GPRX_EINVAL, "null argument");
    if (count == 0) return GPRX_OK;
    HIPCHK(c, hipSetDevice(c->device));
    int rc;
    if ((rc = ensure(c, c->scratch, sizeof(double) * (size_t)count * (c->world + 1)))) return rc;
    double* dsend = c->scratch.p;
    double* drecv = c->scratch.p + count;
    HIPCHK(c, hipMemcpyAsync(dsend, send, sizeof(double) * count, hipMemcpyHostToDevice, c->stream));
    if ((rc = gprx_comm_all_gather(c, dsend, drecv, count))) return rc;
    HIPCHK(c, hipMemcpyAsync(recv, drecv, sizeof(double) * count * c->world, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return GPRX_OK;
  });
}

int gprx_comm_barrier(gprx_comm c) {
  return guarded(c, [&]() -> int {
    if (!c) return fail(c, GPRX_EINVAL, "null communicator");
    int rc;
    HIPCHK(c, hipSetDevice(c->device));
    if ((rc = ensure(c, c->scratch, sizeof(double) * (size_t)(c->world + 1)))) return rc;
    HIPCHK(c, hipMemsetAsync(c->scratch.p, 0, sizeof(double), c->stream));
    if ((rc = gprx_comm_all_reduce_max(c, c->scratch.p, 1))) return rc;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return GPRX_OK;
  });
}

}  // extern "C"
