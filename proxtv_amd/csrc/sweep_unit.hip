// sweep_unit.hip -- the sweep kernels of ONE (op, weighted) pair: compiled seventeen times by proxtv_amd/build.py with
// -DPTV_UNIT_OP=<OpId enumerator> -DPTV_UNIT_W=<true|false> (the pairs of PTV_SWEEP_UNITS in sweep_kernels.hpp).  Every pair
// instantiates its own kernels -- the op is a template parameter of all of them -- so the units share no device code and build in
// parallel; sweep.hip holds the policy state they share (chunk_state()) and dispatches to them.
#include "sweep_kernels.hpp"

#if !defined(PTV_UNIT_OP) || !defined(PTV_UNIT_W)
#error "compile with -DPTV_UNIT_OP=OP_... -DPTV_UNIT_W=true|false (see proxtv_amd/build.py)"
#endif

namespace ptv {
namespace swp {

// unit_launch: the sweep, and its certifier under option certify.
// unit_gated: the mop-up of a kernel that gave some fibres up (pin.hip's level cap): the sequential walk of the flagged fibres only.
// unit_certify: the certifier alone (kernel 4): how many fibres of what a sweep of this op wrote fail the optimality conditions (-1: cannot
// be checked); the failing fibres stay flagged for nobody -- the flags are cleared by the next certified sweep's re-solve or overwritten.
// unit_warm: first use of a device: upload this unit's code object at initialisation, not in the first solve (common.hpp: warm_sweep).
#define PTV_DEFINE_UNIT(ID, W) \
template <> \
void unit_launch<ID, W>(const SweepArgs &args, const FibreGeom &g, hipStream_t stream, bool allow_chunked, int fam) { \
    launch_op_w<ID, W>(args, g, stream, allow_chunked, fam); \
    if (options().certify) launch_certify<ID, W>(args, g, stream); \
} \
 \
template <> \
void unit_gated<ID, W>(const SweepArgs &args, const FibreGeom &g, hipStream_t stream, int *flags) { \
    launch_seq<ID, W>(args, g, stream, true, flags); \
} \
 \
template <> \
long unit_certify<ID, W>(const SweepArgs &args, const FibreGeom &g, hipStream_t stream) { \
    int *flags = nullptr; \
    const long failed = certify_count<ID, W>(args, g, stream, &flags); \
    if (failed > 0) PTV_HIP(hipMemsetAsync(flags, 0, sizeof(int) * (size_t)g.count, stream)); \
    return failed; \
} \
 \
template <> \
void unit_warm<ID, W>() { \
    hipFuncAttributes attr; \
    PTV_HIP(hipFuncGetAttributes(&attr, reinterpret_cast<const void *>((sweep_seq_kernel<ID, W, false>)))); \
}

PTV_DEFINE_UNIT(PTV_UNIT_OP, PTV_UNIT_W)
#ifdef PTV_UNIT_OP2   // a second op in this object (build.py: OP_DR_ROW_FIRST with OP_DR_ROW)
PTV_DEFINE_UNIT(PTV_UNIT_OP2, PTV_UNIT_W)
#endif
#undef PTV_DEFINE_UNIT

}  // namespace swp
}  // namespace ptv
