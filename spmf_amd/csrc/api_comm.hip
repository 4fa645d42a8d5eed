// api_comm.hip -- the row-shard collectives behind the C-ABI (include/spmf_hip.h): the hand-written allreduce over
// peer pointers (spmf_p2p_*; p2p.hip), RCCL bound at run time (spmf_comm_*), and spmf_allreduce over either.
// Host-side orchestration only (ctx.h).
#include <dlfcn.h>
#include <stdio.h>
#include <string.h>

#include "ctx.h"

using namespace spmf;

// ---- RCCL, bound at run time ------------------------------------------------
// The library does not link librccl: single-GPU users never need it.  spmf_comm_*
// dlopen it on first use; the few entry points used are declared here with the
// ABI of <rccl/rccl.h> (ncclUniqueId = 128 opaque bytes, passed by value).
namespace {
struct RcclId { char internal[128]; };
typedef int (*fn_get_id)(RcclId*);
typedef int (*fn_init_rank)(void**, int, RcclId, int);
typedef int (*fn_allreduce)(const void*, void*, size_t, int, int, void*, hipStream_t);
typedef int (*fn_destroy)(void*);
typedef const char* (*fn_errstr)(int);
struct Rccl {
  void* h = nullptr;
  fn_get_id get_id = nullptr;
  fn_init_rank init_rank = nullptr;
  fn_allreduce allreduce = nullptr;
  fn_destroy destroy = nullptr;
  fn_errstr errstr = nullptr;
};
Rccl* rccl() {
  static Rccl r;
  static bool tried = false;
  if (!tried) {
    tried = true;
    for (const char* name : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"}) {
      r.h = dlopen(name, RTLD_NOW | RTLD_GLOBAL);
      if (r.h) break;
    }
    if (r.h) {
      r.get_id = (fn_get_id)dlsym(r.h, "ncclGetUniqueId");
      r.init_rank = (fn_init_rank)dlsym(r.h, "ncclCommInitRank");
      r.allreduce = (fn_allreduce)dlsym(r.h, "ncclAllReduce");
      r.destroy = (fn_destroy)dlsym(r.h, "ncclCommDestroy");
      r.errstr = (fn_errstr)dlsym(r.h, "ncclGetErrorString");
      if (!r.get_id || !r.init_rank || !r.allreduce || !r.destroy) r.h = nullptr;
    }
  }
  return r.h ? &r : nullptr;
}
constexpr int kNcclFloat = 7, kNcclSum = 0;   // ncclFloat32, ncclSum (rccl.h enums)
}  // namespace

// ---- row-shard collective inside the library (spmf_allreduce) ---------
// (1) hand-written, over peer pointers: p2p.hip.  Region layout of a rank:
//     rs[2][kP2PMaxWorld][slice_cap] | ag[2][kP2PMaxWorld][slice_cap] | flags[2][2][kP2PMaxWorld][kP2PMaxChunks] | seq[8]
static void p2p_unmap(spmf_ctx* c) {
  spmf_ctx::P2P& p = c->p2p;
  for (int i = 0; i < p.world; ++i) {
    if (p.peer[i] && p.peer[i] != p.region) (void)hipIpcCloseMemHandle(p.peer[i]);
    p.peer[i] = nullptr;
  }
  p.connected = 0;
}

namespace spmf {

void p2p_release(spmf_ctx* c) {
  spmf_ctx::P2P& p = c->p2p;
  p2p_unmap(c);
  if (p.region) (void)hipFree(p.region);
  p = spmf_ctx::P2P();
}

// spmf_ctx_destroy's end of a context's communicator (c->comm is set)
void comm_release(spmf_ctx* c) {
  Rccl* r = rccl();
  if (r) (void)r->destroy(c->comm);
}

}  // namespace spmf

static int p2p_allreduce(spmf_ctx* c, float* buf, int64_t n, hipStream_t st) {
  spmf_ctx::P2P& p = c->p2p;
  if (n > p.n_max) {
    char b[160];
    snprintf(b, sizeof b, "allreduce: %lld floats, the peer regions were sized for %lld (spmf_p2p_init n_max)",
        (long long)n, (long long)p.n_max);
    return fail(c, SPMF_E_WORKSPACE, b);
  }
  if (((uintptr_t)buf & 15) != 0) return fail(c, SPMF_E_ARG, "allreduce: buffer must be 16-byte aligned");
  if (n == 0 || p.world == 1) return SPMF_OK;
  P2PLaunch L{};
  L.buf = buf;
  L.n = n;
  L.rank = p.rank;
  L.world = p.world;
  L.nchunk = p.nchunk;
  L.slice_cap = p.slice_cap;
  L.rs = (float*)p.region;
  L.ag = (float*)(p.region + p.off_ag);
  L.flags = (uint64_t*)(p.region + p.off_flags);
  L.seq = (uint64_t*)(p.region + p.off_seq);
  for (int i = 0; i < p.world; ++i) {
    L.peer_rs[i] = (float*)p.peer[i];
    L.peer_ag[i] = (float*)(p.peer[i] + p.off_ag);
    L.peer_flags[i] = (uint64_t*)(p.peer[i] + p.off_flags);
  }
  launch_p2p_allreduce(L, st);
  HIPCHK(c, hipGetLastError());
  return SPMF_OK;
}

extern "C" {

int spmf_p2p_init(spmf_ctx* c, int rank, int world, int64_t n_max, int nchunk, void* handle_out64) {
  if (!c || !handle_out64 || world < 1 || world > kP2PMaxWorld || rank < 0 || rank >= world || n_max < 1)
    return fail(c, SPMF_E_ARG, "p2p_init: bad arguments (world <= 16)");
  if (nchunk <= 0) nchunk = 32;
  if (nchunk > kP2PMaxChunks) nchunk = kP2PMaxChunks;
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipDeviceSynchronize());
  spmf_ctx::P2P& p = c->p2p;
  const int64_t per = ((n_max + world - 1) / world + 3) & ~(int64_t)3;
  const int64_t slice_cap = (per + 63) & ~(int64_t)63;           // 256-byte slots
  const size_t box = (size_t)2 * kP2PMaxWorld * slice_cap * sizeof(float);
  const size_t off_flags = 2 * box;
  const size_t off_seq = off_flags + (size_t)2 * 2 * kP2PMaxWorld * kP2PMaxChunks * sizeof(uint64_t);
  const size_t bytes = off_seq + 64;
  // A context's region is allocated ONCE and re-used while it is large enough: freeing a region and exporting a
  // new allocation inside one process is what the runtime's IPC bookkeeping did not survive (round 5, world 4:
  // "hipIpcGetMemHandle: invalid argument", or peers that mapped something stale and never saw a flag).
  p2p_unmap(c);
  char* keep = (p.region && p.alloc_bytes >= bytes) ? p.region : nullptr;
  const size_t keep_bytes = keep ? p.alloc_bytes : 0;
  if (p.region && !keep) (void)hipFree(p.region);
  p = spmf_ctx::P2P();
  p.rank = rank;
  p.world = world;
  p.nchunk = nchunk;
  p.n_max = n_max;
  p.slice_cap = slice_cap;
  p.off_ag = box;
  p.off_flags = off_flags;
  p.off_seq = off_seq;
  p.bytes = bytes;
  hipError_t e = hipSuccess;
  if (keep) {
    p.region = keep;
    p.alloc_bytes = keep_bytes;
  } else {
    // fine-grained: coherent across agents INSIDE a kernel (a coarse-grained allocation is only
    // coherent at kernel boundaries); what RCCL allocates for its own buffers
    void* reg = nullptr;
    e = hipExtMallocWithFlags(&reg, p.bytes, hipDeviceMallocFinegrained);
    if (e != hipSuccess) {
      (void)hipGetLastError();
      return fail(c, SPMF_E_HIP, std::string("p2p_init: hipExtMallocWithFlags(fine-grained): ") + hipGetErrorString(e));
    }
    p.region = (char*)reg;
    p.alloc_bytes = p.bytes;
  }
  HIPCHK(c, hipMemset(p.region + p.off_flags, 0, p.bytes - p.off_flags));
  HIPCHK(c, hipDeviceSynchronize());
  hipIpcMemHandle_t hnd;
  static_assert(sizeof(hipIpcMemHandle_t) == 64, "spmf_p2p_init hands out 64-byte handles");
  e = hipIpcGetMemHandle(&hnd, p.region);
  if (e != hipSuccess) {
    // seen once (round 5, world 4, a region re-created in a process whose earlier region a peer had still mapped
    // when it was freed): the runtime refused to export the new allocation.  One more try at another address.
    (void)hipGetLastError();
    void* again = nullptr;
    if (hipExtMallocWithFlags(&again, p.bytes, hipDeviceMallocFinegrained) == hipSuccess) {
      (void)hipFree(p.region);
      p.region = (char*)again;
      p.alloc_bytes = p.bytes;
      (void)hipMemset(p.region + p.off_flags, 0, p.bytes - p.off_flags);
      (void)hipDeviceSynchronize();
      e = hipIpcGetMemHandle(&hnd, p.region);
    }
  }
  if (e != hipSuccess) {
    (void)hipGetLastError();
    p2p_release(c);
    return fail(c, SPMF_E_HIP, std::string("p2p_init: hipIpcGetMemHandle: ") + hipGetErrorString(e));
  }
  memcpy(handle_out64, &hnd, 64);
  return SPMF_OK;
}

int spmf_p2p_connect(spmf_ctx* c, const void* handles) {
  if (!c || !handles) return fail(c, SPMF_E_ARG, "p2p_connect: bad arguments");
  spmf_ctx::P2P& p = c->p2p;
  if (!p.region) return fail(c, SPMF_E_ARG, "p2p_connect: spmf_p2p_init was not called");
  HIPCHK(c, hipSetDevice(c->device));
  for (int i = 0; i < p.world; ++i) {
    if (i == p.rank) {
      p.peer[i] = p.region;
      continue;
    }
    hipIpcMemHandle_t hnd;
    memcpy(&hnd, (const char*)handles + (size_t)i * 64, 64);
    void* ptr = nullptr;
    const hipError_t e = hipIpcOpenMemHandle(&ptr, hnd, hipIpcMemLazyEnablePeerAccess);
    if (e != hipSuccess) {
      (void)hipGetLastError();
      char b[200];
      snprintf(b, sizeof b, "p2p_connect: hipIpcOpenMemHandle(rank %d): %s", i, hipGetErrorString(e));
      return fail(c, SPMF_E_HIP, b);
    }
    p.peer[i] = (char*)ptr;
    // a region that lives on ANOTHER device of this process's view (ranks = GPUs of one node): kernels here will
    // store into it, so the link must be there -- an inaccessible peer is refused now (the caller falls back to
    // RCCL: dist.PeerComm agrees on the failure over all ranks) instead of faulting in the first launch.
    // Same device (ranks = processes on one GPU: the one-GPU tests) or attributes unavailable: nothing to check.
    hipPointerAttribute_t at;
    if (hipPointerGetAttributes(&at, ptr) == hipSuccess) {
      if (at.device >= 0 && at.device != c->device) {
        int can = 0;
        if (hipDeviceCanAccessPeer(&can, c->device, at.device) == hipSuccess && !can) {
          char b[200];
          snprintf(b, sizeof b, "p2p_connect: device %d has no peer access to device %d (rank %d)", c->device,
                   at.device, i);
          return fail(c, SPMF_E_UNSUPPORTED, b);
        }
      }
    } else {
      (void)hipGetLastError();
    }
  }
  p.connected = 1;
  return SPMF_OK;
}

int spmf_p2p_enable(spmf_ctx* c, int on) {
  if (!c) return SPMF_E_ARG;
  if (on && (!c->p2p.region || !c->p2p.peer[c->p2p.world > 0 ? c->p2p.world - 1 : 0]))
    return fail(c, SPMF_E_ARG, "p2p_enable: spmf_p2p_connect has not connected the peers");
  c->p2p.connected = on ? 1 : 0;
  return SPMF_OK;
}

int spmf_p2p_status(spmf_ctx* c, uint64_t out3[3]) {
  if (!c || !out3) return SPMF_E_ARG;
  if (!c->p2p.region) return fail(c, SPMF_E_ARG, "p2p_status: spmf_p2p_init was not called");
  HIPCHK(c, hipDeviceSynchronize());
  HIPCHK(c, hipMemcpy(out3, c->p2p.region + c->p2p.off_seq, 3 * sizeof(uint64_t), hipMemcpyDeviceToHost));
  return SPMF_OK;
}

int spmf_p2p_disconnect(spmf_ctx* c) {
  if (!c) return SPMF_E_ARG;
  (void)hipDeviceSynchronize();
  p2p_unmap(c);
  return SPMF_OK;
}

int spmf_p2p_destroy(spmf_ctx* c) {
  if (!c) return SPMF_E_ARG;
  (void)hipDeviceSynchronize();
  p2p_release(c);
  return SPMF_OK;
}

// (2) RCCL, bound at run time
int spmf_comm_unique_id(void* out128) {
  if (!out128) return SPMF_E_ARG;
  Rccl* r = rccl();
  if (!r) return SPMF_E_UNSUPPORTED;
  RcclId id;
  const int rc = r->get_id(&id);
  if (rc != 0) return SPMF_E_HIP;
  memcpy(out128, &id, sizeof id);
  return SPMF_OK;
}

int spmf_comm_init(spmf_ctx* c, const void* id128, int rank, int world) {
  if (!c || !id128 || world < 1 || rank < 0 || rank >= world) return fail(c, SPMF_E_ARG, "comm_init: bad arguments");
  Rccl* r = rccl();
  if (!r) return fail(c, SPMF_E_UNSUPPORTED, "comm_init: librccl.so.1 could not be loaded");
  if (c->comm) {
    (void)r->destroy(c->comm);
    c->comm = nullptr;
  }
  HIPCHK(c, hipSetDevice(c->device));
  RcclId id;
  memcpy(&id, id128, sizeof id);
  void* comm = nullptr;
  const int rc = r->init_rank(&comm, world, id, rank);
  if (rc != 0) return fail(c, SPMF_E_HIP, std::string("ncclCommInitRank: ") + (r->errstr ? r->errstr(rc) : "?"));
  c->comm = comm;
  c->comm_rank = rank;
  c->comm_world = world;
  return SPMF_OK;
}

int spmf_allreduce(spmf_ctx* c, float* buf, int64_t n, void* stream) {
  if (!c || !buf || n < 0) return fail(c, SPMF_E_ARG, "allreduce: bad arguments");
  if (c->p2p.connected) return p2p_allreduce(c, buf, n, (hipStream_t)stream);
  if (!c->comm) return fail(c, SPMF_E_ARG, "allreduce: neither spmf_comm_init nor spmf_p2p_connect was called");
  if (n == 0) return SPMF_OK;
  Rccl* r = rccl();
  const int rc = r->allreduce(buf, buf, (size_t)n, kNcclFloat, kNcclSum, c->comm, (hipStream_t)stream);
  if (rc != 0) return fail(c, SPMF_E_HIP, std::string("ncclAllReduce: ") + (r->errstr ? r->errstr(rc) : "?"));
  return SPMF_OK;
}

int spmf_comm_destroy(spmf_ctx* c) {
  if (!c) return SPMF_E_ARG;
  if (c->comm) {
    Rccl* r = rccl();
    if (r) (void)r->destroy(c->comm);
    c->comm = nullptr;
    c->comm_world = 1;
    c->comm_rank = 0;
  }
  return SPMF_OK;
}

}  // extern "C"
