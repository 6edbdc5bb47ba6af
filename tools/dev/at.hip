// development translation unit: the atile kernels alone
#include "srx_prims.hpp"
#include "srx_fused.hpp"
#include "srx_mosaic.hpp"
#include "srx_patch.hpp"
#include "srx_btile.hpp"
#include "srx_atile.hpp"
namespace srx { Profiler &profiler() { static Profiler p; return p; } }
int dummy(srx::Arena &ar, const srx::mosaic::Common<float> &c, const float *p, float *q, double *e)
{
    return srx::atile::iterate(c, p, q, 2, e, ar, 0);
}
