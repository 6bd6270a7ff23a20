// The host side between an extern "C" entry point and <<< >>>: the one launch form of the kernels that may need more than 64 KB of dynamic
// LDS, and the dropout decision every argument fill states.  An entry point fills a call record (the *Call structs next to the static
// implementations: every field null / zero by default, the entry names what it supplies), the implementation checks it, fills the kernel's
// argument struct and launches through launch_lds.  AMID_LAUNCH_CHECK stays the form of the launches without large LDS.
#pragma once
#include "common.h"
#include "rng.h"

namespace amid {

// a family: a host array of device pointers ([domain], or [layer][domain]) as the entry points take them; read-only / written tensors
using FamC = const float* const*;
using Fam = float* const*;

// raise the kernel's dynamic-LDS limit once per device (common.h lds_attr_once), launch, read the launch's error.  The kernel is a template
// parameter: one instantiation, hence one per-device mask, per kernel.  `lds` must be the same in every call for a given kernel (every
// call site passes the kernel's compile-time size): the limit is raised to the FIRST call's size on a device and not looked at again.
template <auto KERNEL, class... Args>
static int launch_lds(int grid, int block, size_t lds, void* stream, const Args&... args) {
    static unsigned long long attr_done = 0;
    if (int rc = lds_attr_once((const void*)KERNEL, lds, attr_done)) return rc;
    KERNEL<<<grid, block, lds, (hipStream_t)stream>>>(args...);
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? AMID_OK : (int)e;
}

// what a dropout site is given: it draws only in a training step with p > 0; spec = the keep decisions' width and threshold (rng.h
// drop_spec), scale = 1 / (1 - p) on the kept elements
struct DropoutArgs { int train; unsigned spec; float scale; };
static inline DropoutArgs dropout_args(int train, float p_drop) {
    DropoutArgs d;
    d.train = (train && p_drop > 0.f) ? 1 : 0;
    d.spec = drop_spec(p_drop);
    d.scale = d.train ? 1.0f / (1.0f - p_drop) : 1.0f;
    return d;
}

}  // namespace amid
