// esim_api.hip -- host side of libesim: the C ABI of include/esim.h over the kernels of esim_kernels.hip.  No CPU compute
// path exists here: without a HIP device every entry point that would compute fails with ESIM_ENODEVICE.
// One translation unit, in parts by concern (esim_host_*.h: each part's first lines say what it holds).
#include "esim_kernels.hip"

#include <dlfcn.h>
#include <rccl/rccl.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <string>
#include <thread>
#include <vector>

#include "esim_host_ctx.h"
#include "esim_host_ensemble.h"
#include "esim_host_members.h"
#include "esim_host_depth.h"
#include "esim_host_dist.h"
#include "esim_host_arms.h"
#include "esim_host_merge.h"
#include "esim_host_upload.h"
#include "esim_host_run.h"
#include "esim_host_shard.h"
#include "esim_host_outputs.h"
#include "esim_host_settings.h"
#include "esim_host_tree.h"
#include "esim_host_ensrows.h"
#include "esim_host_compare.h"
#include "esim_host_household.h"
#include "esim_host_places.h"
#include "esim_host_contacts.h"
#include "esim_host_flows.h"
#include "esim_host_curves.h"
#include "esim_host_burden.h"
#include "esim_host_beds.h"
#include "esim_host_events.h"
#include "esim_host_ckpt.h"
#include "esim_host_snapshot.h"
#include "esim_host_timing.h"
