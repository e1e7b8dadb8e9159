// k_ingest_pack_g1.hip -- k_ingest_pack instantiations of the 256 x 16 geometry, one per key-hash kind
#include "fw_ingest_pack.h"

namespace fw {
hipError_t launch_ingest_pack_g1(const IngestArgs& a, hipStream_t s, KTimer* t) {
    return ingest_pack_geom<IGP_BLOCK1, IGP_RPT1, IGP_WAVES1>(a, s, t);
}
int ingest_pack_occupancy_g1() { return ingest_pack_wg_per_cu<IGP_BLOCK1, IGP_RPT1, IGP_WAVES1>(); }
}  // namespace fw
