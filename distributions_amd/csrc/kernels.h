// HIP kernels of libdistributions_hip (gfx950).  Included once, by
// dist_hip.hip.  Layout and roofline notes per kernel are in DESIGN.md.
#pragma once

#include <type_traits>

#include "models.h"

namespace dist {

constexpr int kBlock = 256;
constexpr int kMaxF = DIST_MAX_FEATURES;

// Dynamic LDS.  Each kernel that takes some has its size function beside it
// (<kernel>_lds): the host's eligibility tests and launches call that and
// compute no byte count of their own.  Up to kLdsNoOptIn bytes a launch needs
// nothing more; beyond, the kernel instance opts in first (launch_lds,
// dist_hip.hip).  A 1024-thread workgroup may take most of the CU's 160 KiB:
// kLdsWorkgroupLimit.
constexpr size_t kLdsNoOptIn = 64 * 1024;
constexpr size_t kLdsWorkgroupLimit = 144 * 1024;

}  // namespace dist

// (split by path; the order matters: later parts use the earlier ones)
#include "kernels_api.h"
#include "kernels_rows.h"
#include "kernels_predict.h"
#include "kernels_ensemble.h"
#include "kernels_coassign.h"
#include "kernels_coassign_topk.h"
#include "kernels_feature.h"
#include "kernels_marginals.h"
#include "kernels_sample.h"
#include "kernels_sample_many.h"
#include "kernels_vs.h"
#include "kernels_apply.h"
#include "kernels_hyper.h"
#include "kernels_partitions.h"
#include "kernels_search.h"
