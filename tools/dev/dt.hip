// development translation unit: the dtile kernels alone (fast compile, resource usage)
#include "srx_prims.hpp"
#include "srx_fused.hpp"
#include "srx_mosaic.hpp"
#include "srx_patch.hpp"
#include "srx_dtile.hpp"
namespace srx { Profiler &profiler() { static Profiler p; return p; } }
int dummy(srx::Arena &ar, const srx::mosaic::Common<float> &c, const float *p, float *q, double *e)
{
    return srx::dtile::iterate(c, p, q, 2, e, ar, 0);
}
