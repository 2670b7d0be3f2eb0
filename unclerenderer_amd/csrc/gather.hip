// The row-band all-gather of include/ur_hotpath.h over RCCL, which is looked up at run time. Host code only.

#include <dlfcn.h>

#include "ur_internal.h"

using ur::set_error;

typedef int (*nccl_allgather_fn)(const void*, void*, size_t, int, void*, hipStream_t);

// RCCL is resolved at run time from whatever copy the host process already loaded globally (the communicator must come
// from the same copy), falling back to the system's librccl: the library has no link-time dependency on RCCL.
static void* rccl_symbol(const char* name)
{
    void* fn = dlsym(RTLD_DEFAULT, name);
    if (!fn) {
        static void* lib = nullptr;
        if (!lib) lib = dlopen("librccl.so", RTLD_NOW | RTLD_GLOBAL);
        if (!lib) lib = dlopen("librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
        if (lib) fn = dlsym(lib, name);
    }
    return fn;
}

extern "C" {

int ur_allgather_rows_bytes_ex(ur_ctx* ctx, void* comm, void* image, uint32_t row_bytes, uint32_t h, uint32_t n_ranks, uint32_t rank, int mode)
{
    if (!ctx || !comm || !image || row_bytes == 0 || h == 0 || n_ranks == 0 || rank >= n_ranks || h % n_ranks != 0) {
        set_error("ur_allgather_rows: bad argument (row_bytes=%u h=%u ranks=%u rank=%u)", row_bytes, h, n_ranks, rank);
        return UR_EINVAL;
    }
    if (mode != UR_GATHER_RING && mode != UR_GATHER_DIRECT) { set_error("ur_allgather_rows: mode %d (0 ring, 1 direct)", mode); return UR_EINVAL; }
    const size_t band_bytes = (size_t)row_bytes * (h / n_ranks);
    char* base = reinterpret_cast<char*>(image);
    const char* send = base + band_bytes * rank;
    if (mode == UR_GATHER_RING) {
        static nccl_allgather_fn fn = nullptr;
        if (!fn) fn = reinterpret_cast<nccl_allgather_fn>(rccl_symbol("ncclAllGather"));
        if (!fn) { set_error("ur_allgather_rows: ncclAllGather not found"); return UR_EUNSUPPORTED; }
        const int rc = fn(send, image, band_bytes, /*ncclInt8*/ 0, comm, ctx->stream);
        if (rc != 0) { set_error("ncclAllGather failed (%d)", rc); return UR_EHIP; }
        return UR_OK;
    }
    // Direct form: the band goes to every peer over the xGMI link the two GPUs share (an MI355X node is fully connected,
    // 7 links per GPU), all N - 1 transfers of a rank in flight at once — one grouped call, no ring hops.
    typedef int (*group_fn)(void);
    typedef int (*send_fn)(const void*, size_t, int, int, void*, hipStream_t);
    typedef int (*recv_fn)(void*, size_t, int, int, void*, hipStream_t);
    static group_fn g_start = nullptr, g_end = nullptr;
    static send_fn f_send = nullptr;
    static recv_fn f_recv = nullptr;
    if (!g_start) {
        g_start = reinterpret_cast<group_fn>(rccl_symbol("ncclGroupStart"));
        g_end = reinterpret_cast<group_fn>(rccl_symbol("ncclGroupEnd"));
        f_send = reinterpret_cast<send_fn>(rccl_symbol("ncclSend"));
        f_recv = reinterpret_cast<recv_fn>(rccl_symbol("ncclRecv"));
    }
    if (!g_start || !g_end || !f_send || !f_recv) { g_start = nullptr; set_error("ur_allgather_rows: ncclGroupStart/End, ncclSend, ncclRecv not found"); return UR_EUNSUPPORTED; }
    int rc = g_start();
    // peers in the order rank + 1, rank + 2, ...: at any moment every rank sends to a different peer
    for (uint32_t k = 1; k < n_ranks && rc == 0; ++k) {
        const uint32_t to = (rank + k) % n_ranks, from = (rank + n_ranks - k) % n_ranks;
        rc = f_send(send, band_bytes, /*ncclInt8*/ 0, (int)to, comm, ctx->stream);
        if (rc == 0) rc = f_recv(base + band_bytes * from, band_bytes, /*ncclInt8*/ 0, (int)from, comm, ctx->stream);
    }
    const int rc_end = g_end();
    if (rc != 0 || rc_end != 0) { set_error("grouped ncclSend/ncclRecv failed (%d, %d)", rc, rc_end); return UR_EHIP; }
    return UR_OK;
}

int ur_allgather_rows_bytes(ur_ctx* ctx, void* comm, void* image, uint32_t row_bytes, uint32_t h, uint32_t n_ranks, uint32_t rank)
{
    return ur_allgather_rows_bytes_ex(ctx, comm, image, row_bytes, h, n_ranks, rank, UR_GATHER_RING);
}

int ur_allgather_rows(ur_ctx* ctx, void* comm, ur_half4* hdr_full, uint32_t w, uint32_t h, uint32_t n_ranks, uint32_t rank)
{
    if ((uint64_t)w * sizeof(ur_half4) > 0xFFFFFFFFull) { set_error("ur_allgather_rows: row of %u pixels is too wide", w); return UR_EINVAL; }
    return ur_allgather_rows_bytes(ctx, comm, hdr_full, w * (uint32_t)sizeof(ur_half4), h, n_ranks, rank);
}

} // extern "C"
