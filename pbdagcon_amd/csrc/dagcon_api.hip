// dagcon_api.hip -- host side of the C ABI (include/dagcon.h).
//
// Owns the HIP stream, the HBM arenas and the launch sequence of the hot path
//   a1 k_norm_*             | a2 k_carve, k_groups, k_emit, k_lists |
//   b  k_merge              | c  k_bestpath
// There is no CPU fallback anywhere in it: without a HIP device
// dagcon_create fails with DAGCON_ERR_NO_DEVICE.
// One translation unit, cut by stage into the five api_* files included below; api_outputs.hip.h holds the host side of
// every optional output of a run (its room, parameters, launches, fetch and entry points).
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <chrono>
#include <array>
#include <vector>

#include "../../include/dagcon.h"
#include "dagcon_dev.h"
#include "k_build.hip.h"
#include "k_merge.hip.h"
#include "k_merge_q.hip.h"
#include "k_bestpath.hip.h"
#include "k_align.hip.h"
#include "k_align_panels.hip.h"
#include "k_place.hip.h"
#include "k_cigar.hip.h"
#include "k_rate.hip.h"
#include "k_cs.hip.h"
#include "k_md.hip.h"
#include "k_edits.hip.h"
#include "k_evidence.hip.h"
#include "k_pileup.hip.h"
#include "k_site_reads.hip.h"
#include "k_site_link.hip.h"
#include "k_hap.hip.h"
#include "k_hap_calls.hip.h"
#include "k_alleles.hip.h"
#include "k_join.hip.h"
#include "k_winlink.hip.h"
#include "k_keep.hip.h"
#include "host/alleles.h"
#include "api_ctx.h"
#include "api_run.hip.h"
#include "api_outputs.hip.h"
#include "api_align.hip.h"
#include "api_records.hip.h"
