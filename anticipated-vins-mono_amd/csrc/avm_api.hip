// avm_api.hip — the C ABI of include/avm.h on top of the gfx950 kernels.
// Host language is C++ (the reference's host code is C++: vins_estimator/src/estimator.cpp,
// feature_selector.cpp).  No torch types, no exceptions across the boundary.  There is no CPU
// fallback: without a HIP device avm_create() fails with AVM_ERR_NO_DEVICE.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <string>
#include <type_traits>
#include <vector>

#include <dlfcn.h>
#include <rccl/rccl.h>  // types only: the library is dlopen'ed (avm_comm_*), a single-GPU host never needs it

#include "kernels.hpp"
#include "select_image.hpp"

using namespace avm;

// The parts of this translation unit, by subsystem (one object: the helpers live in anonymous namespaces and need no declarations)
#include "api/ctx.hpp"
#include "api/comm.hpp"
#include "api/checks.hpp"
#include "api/fields.hpp"
#include "api/staging.hpp"
#include "api/preint.hpp"
#include "api/solve.hpp"
#include "api/window_ops.hpp"
#include "api/tracks.hpp"
#include "api/relo.hpp"
#include "api/align.hpp"
#include "api/sfm.hpp"
#include "api/fsel.hpp"
#include "api/debug.hpp"
