// k_ingest_pack.hip -- k_ingest_pack instantiations of the 512 x 8 geometry, one per key-hash kind, and
// the launcher that chooses the geometry (the 256 x 16 instantiations: k_ingest_pack_g1.hip)
#include "fw_ingest_pack.h"

namespace fw {
// k_ingest leaves the report to this one-thread launch (its registers are full: fw_ingest_impl.h); the
// host queues it behind a k_ingest push of a handle that chooses between the two kernels
__global__ void k_ig_report(const Tickets* tk, const Ctrl* ctrl) { ig_mirror_store(tk, ctrl); }
hipError_t launch_ig_report(const Tickets* tk, const Ctrl* ctrl, hipStream_t s) {
    hipLaunchKernelGGL(k_ig_report, dim3(1), dim3(1), 0, s, tk, ctrl);
    return hipGetLastError();
}

hipError_t launch_ingest_pack(const IngestArgs& a, int geom, hipStream_t s, KTimer* t) {
    return geom ? launch_ingest_pack_g1(a, s, t) : ingest_pack_geom<IGP_BLOCK, IGP_RPT, IGP_WAVES>(a, s, t);
}
int ingest_pack_occupancy(int geom) {
    return geom ? ingest_pack_occupancy_g1() : ingest_pack_wg_per_cu<IGP_BLOCK, IGP_RPT, IGP_WAVES>();
}
}  // namespace fw
