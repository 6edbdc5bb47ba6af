// development translation unit: the strip kernels alone (fast compile, resource usage)
#include "srx_prims.hpp"
#include "srx_fused.hpp"
#include "srx_mosaic.hpp"
#include "srx_patch.hpp"
#include "srx_stile.hpp"
namespace srx { Profiler &profiler() { static Profiler p; return p; } }
int dummy(srx::Arena &ar, const srx::mosaic::Common<double> &c, const double *p, double *q, double *e)
{
    return srx::stile::iterate<double>(c, p, q, 2, e, ar, 0);
}
