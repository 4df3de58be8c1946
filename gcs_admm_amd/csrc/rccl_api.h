// rccl_api.h -- RCCL, bound at run time (used by gcsadmm.hip: the halo exchange and the all-reduce of a vertex partition).
// The library is not linked against librccl: a process that already carries an RCCL (PyTorch-ROCm ships its own copy with the
// SONAME of /opt/rocm's) must not end up with two, and a single-GPU user needs none.  dlopen returns the copy that is already
// loaded, or loads the system one.  Host code only.
#pragma once
#include <dlfcn.h>
#include <rccl/rccl.h>

#include <string>

#include "gcsadmm.h"

namespace {
struct RcclApi {
    void *lib = nullptr;
    decltype(&ncclGetUniqueId) GetUniqueId = nullptr;
    decltype(&ncclCommInitRank) CommInitRank = nullptr;
    decltype(&ncclCommDestroy) CommDestroy = nullptr;
    decltype(&ncclGroupStart) GroupStart = nullptr;
    decltype(&ncclGroupEnd) GroupEnd = nullptr;
    decltype(&ncclSend) Send = nullptr;
    decltype(&ncclRecv) Recv = nullptr;
    decltype(&ncclAllReduce) AllReduce = nullptr;
    decltype(&ncclGetErrorString) GetErrorString = nullptr;
    decltype(&ncclCommCount) CommCount = nullptr;
    std::string err;
    bool ok() const { return lib && GetUniqueId && CommInitRank && CommDestroy && GroupStart && GroupEnd && Send && Recv && AllReduce; }
    const char *text(ncclResult_t r) const { return GetErrorString ? GetErrorString(r) : "RCCL error"; }
};
RcclApi &rccl()
{
    static RcclApi api = [] {
        RcclApi a;
        for (const char *name : {"librccl.so.1", "librccl.so"}) {
            a.lib = dlopen(name, RTLD_NOW | RTLD_GLOBAL);
            if (a.lib) break;
        }
        if (!a.lib) {
            const char *why = dlerror();      // (a second call would return NULL: the message is consumed)
            a.err = std::string("dlopen(librccl): ") + (why ? why : "not found");
            return a;
        }
#define RCCL_SYM(f) a.f = (decltype(a.f))dlsym(a.lib, "nccl" #f)
        RCCL_SYM(GetUniqueId); RCCL_SYM(CommInitRank); RCCL_SYM(CommDestroy); RCCL_SYM(GroupStart); RCCL_SYM(GroupEnd);
        RCCL_SYM(Send); RCCL_SYM(Recv); RCCL_SYM(AllReduce); RCCL_SYM(GetErrorString); RCCL_SYM(CommCount);
#undef RCCL_SYM
        if (!a.ok()) a.err = "librccl lacks an expected symbol";
        return a;
    }();
    return api;
}
}  // namespace

// of one family with HIPCHK (gcsadmm.hip): `obj` is the handle or batch whose err takes the text
#define NCCLCHK(obj, call)                                                                           \
    do {                                                                                             \
        ncclResult_t r_ = (call);                                                                    \
        if (r_ != ncclSuccess) {                                                                     \
            (obj)->err = std::string(#call) + ": " + rccl().text(r_);                                \
            return GCSADMM_ERR_HIP;                                                                  \
        }                                                                                            \
    } while (0)
