// nt_step_preamble.hpp -- what every stepping translation unit (nt_kernels.hip: collide / XPBD / SemiImplicit; nt_featherstone.hip:
// SolverFeatherstone + eval_fk) starts with: the math helpers in both arithmetic namespaces, the LDS layout, the per-lane context and
// the phase headers, inside one anonymous namespace per unit.  Two units because their kernels want different compilers: the XPBD
// rollouts gain 5 % from LLVM's iterative ILP scheduling strategy, SolverFeatherstone's lose 13 % to it (profiles/r06E_ab_workloads.txt)
// -- and the strategy is a per-unit option (__graft_entry__.UNIT_FLAGS).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <type_traits>

#include "../../include/newton_hip.h"
#include "nt_math.hpp"
#include "nt_primitives.hpp"
#include "nt_convex.hpp"

// Two arithmetic namespaces in one translation unit (the fused kernels run both on the same LDS tile):
//  * ieee  -- nt:: helpers, -ffp-contract=off, correctly rounded division / sqrt: everything that decides pair sets, contact
//             counts and contact geometry (shape transforms, AABBs, broad phase, primitive / MPR-GJK narrow phase, the contact
//             writer), SolverSemiImplicit and SolverFeatherstone.  CollisionPipeline.collide stays bit-identical to the contact
//             arrays the reference's own kernels produce (tests/golden/collide_reference_vectors.npz).
//  * fused -- ntf:: helpers (a second copy of nt_math.hpp) + the XPBD phases of nt_xpbd.hpp under `#pragma clang fp
//             contract(fast)` and -DNT_XPBD_FAST_MATH: a * b + c contracts to v_fma_f32, the divisions / square roots of the
//             projection phases are v_rcp_f32 / v_sqrt_f32 (1 ulp).  Within SURVEY.md 8(c)'s contract (1e-5 single step, 1e-4
//             rollout against the reference); measured on the MI355X headline: 0.363 -> 0.308 ms per 10-substep launch for the whole
//             kernel (profiles/r04a_*).  clang attaches the contraction permission to an operation where it is WRITTEN, hence the
//             second copy of the helpers instead of a flag.
// The step and the rollout kernels share the fused phases, so a rollout stays bitwise equal to the call-by-call loop.
// -DNT_XPBD_IEEE (measurement builds only, tools/build_variant.py): the XPBD phases with IEEE arithmetic -- no contraction, correctly
// rounded division / square root, the literal rotation formulas -- to measure what the fast arithmetic contributes to the threshold
// events of an open-loop frame (tests/tolerances.py: explain_rollout_outliers).
#define NT_MATH_NS ntf
#ifndef NT_XPBD_IEEE
#pragma clang fp contract(fast)
#endif
#include "nt_math.hpp"
#pragma clang fp contract(off)
#undef NT_MATH_NS

namespace {

#include "nt_layout.hpp"

namespace ieee {
using namespace nt;
#include "nt_ctx.hpp"
#include "nt_collide.hpp"
#include "nt_xpbd.hpp"
#define NT_SI_PHASES_ONLY  // (the SolverSemiImplicit kernel itself follows below, once)
#include "nt_semi_implicit.hpp"
#undef NT_SI_PHASES_ONLY
#include "nt_featherstone.hpp"
}  // namespace ieee

#ifndef NT_XPBD_IEEE
#pragma clang fp contract(fast)
#define NT_XPBD_FAST_MATH
#endif
namespace fused {
using namespace ntf;
#include "nt_ctx.hpp"
#include "nt_xpbd.hpp"
}  // namespace fused
#undef NT_XPBD_FAST_MATH
#pragma clang fp contract(off)

namespace ieee {
#include "nt_xpbd_kernels.hpp"
#define NT_SI_KERNEL_ONLY
#include "nt_semi_implicit.hpp"
#undef NT_SI_KERNEL_ONLY
#include "nt_featherstone_kernels.hpp"
}  // namespace ieee
using namespace ieee;

constexpr size_t LDS_BYTES_PER_CU = 160 * 1024;

bool model_ok(const nt_model* m) {
    return m && m->env_count > 0 && m->env_stride >= m->env_count && (m->env_stride % 64) == 0 && m->nb > 0 &&
           (m->cpp == 4 || m->cpp == 5) && m->np_analytic >= 0 && m->np_analytic <= m->np &&
           (m->np_analytic == m->np || m->cpp == 5);
}

// ------------------------------------------------------------------------------------------------
// tile launch (every stepping kernel: one workgroup owns `epb` environments, KArgs::nslot slot-lanes each)
// ------------------------------------------------------------------------------------------------
// LDS bytes of a tile: `rows` floats per environment (LdsLayout / FsLayout rows), then the block-shared ints (topology) and floats
// (the one parameter copy of a uniform-parameter tile)
inline size_t tile_bytes(int rows, int epb, size_t shared_ints, int uni_floats = 0) {
    return (size_t)rows * 4 * epb + shared_ints * 4 + (size_t)uni_floats * 4;
}

// workgroup size: the slot-lanes of `epb` environments, in whole waves
inline int tile_threads(int nslot, int epb) { return ((nslot * epb + 63) / 64) * 64; }

// the phase-ablation mask of measurement builds (-DNT_ABLATION), read once per process
#ifdef NT_ABLATION
inline int debug_skip() {
    static int dbg = -1;
    if (dbg < 0) { const char* e = getenv("NT_DEBUG_SKIP"); dbg = e ? atoi(e) : 0; }
    return dbg;
}
#endif

// one workgroup per `epb` environments, a.nslot slot-lanes each, `lds_bytes` of dynamic LDS (opted in above the 48 KB default);
// `extra`: the kernel's arguments behind KArgs
// NT_TILE_IMAGE=0: the launch goes without the tile image (nt_model.tile_image_words = 0) (the kernels stage the block-shared region from the descriptor's own
// tables) -- the A/B of the two staging paths within one library, and what the tests hold the image against
inline bool tile_image_enabled() {
    const char* e = getenv("NT_TILE_IMAGE");
    return !(e && e[0] == '0' && e[1] == 0);
}
template <typename K, typename... A>
nt_status launch_tile(K kernel, KArgs a, int epb, size_t lds_bytes, hipStream_t stream, A... extra) {
    if (!tile_image_enabled()) a.m.tile_image_words = 0;  // (body_flags stays what it is: the image's first table)
#ifdef NT_ABLATION
    a.debug_skip = debug_skip();
#endif
    if (lds_bytes > 48 * 1024 &&
        hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes) != hipSuccess)
        return NT_ERR_LAUNCH;
    hipLaunchKernelGGL(kernel, dim3((a.m.env_count + epb - 1) / epb), dim3(tile_threads(a.nslot, epb)), lds_bytes, stream, a, extra...);
    return hipGetLastError() == hipSuccess ? NT_OK : NT_ERR_LAUNCH;
}

// runtime environments per workgroup -> compiled instantiation: f(std::integral_constant<int, E>) for the E of the list equal to
// `epb`; NT_ERR_UNSUPPORTED when none is (each call site maps its runtime values onto its list first)
template <int... Es>
struct Epbs {};
template <int... Es, typename F>
nt_status dispatch_epb(Epbs<Es...>, int epb, F&& f) {
    nt_status r = NT_ERR_UNSUPPORTED;
    (void)((epb == Es && ((r = f(std::integral_constant<int, Es>{})), true)) || ...);
    return r;
}

}  // namespace
