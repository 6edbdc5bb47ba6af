// development translation unit: the btile kernels alone (fast compile, resource usage)
#include "srx_prims.hpp"
#include "srx_fused.hpp"
#include "srx_mosaic.hpp"
#include "srx_patch.hpp"
#include "srx_btile.hpp"
namespace srx { Profiler &profiler() { static Profiler p; return p; } }
int dummy(const srx::IbpCall<float> &c) { return srx::btile::ibp(c); }
