// k_ingest_pack.hip -- k_ingest_pack instantiations, one per key-hash kind
#include "fw_ingest_pack.h"

namespace fw {
// k_ingest leaves the report to this one-thread launch (its registers are full: fw_ingest_impl.h); the
// host queues it behind a k_ingest push of a handle that chooses between the two kernels
__global__ void k_ig_report(const Tickets* tk, const Ctrl* ctrl) { ig_mirror_store(tk, ctrl); }
hipError_t launch_ig_report(const Tickets* tk, const Ctrl* ctrl, hipStream_t s) {
    hipLaunchKernelGGL(k_ig_report, dim3(1), dim3(1), 0, s, tk, ctrl);
    return hipGetLastError();
}

hipError_t launch_ingest_pack(const IngestArgs& a, hipStream_t s, KTimer* t) {
    if (a.n_chunks == 0) return hipSuccess;
    if (!igp_serves(a)) return hipErrorInvalidValue;
    switch (a.ks.hash_kind) {
        case KH_LONG: return ingest_pack_hk<KH_LONG>(a, s, t);
        case KH_INT: return ingest_pack_hk<KH_INT>(a, s, t);
        case KH_BINROW_BIGINT: return ingest_pack_hk<KH_BINROW_BIGINT>(a, s, t);
        default: return ingest_pack_hk<KH_BINROW_INT>(a, s, t);
    }
}
}  // namespace fw
