// curve_banderwagon.hip -- instantiates the MSM kernels and engine for Banderwagon (twisted Edwards, ec.h; one TU per curve keeps builds parallel).
#include "hip_backend.h"
#ifdef CTT_TU_ACCUM_INTO   // (the second build of this file, into_banderwagon.o: the accumulate kernel's INTO form only -- hip_backend.h)
template void ctt::launch_accum_into<ctt::Banderwagon::FD>(hipStream_t, const ctt::AccumArgs<ctt::Banderwagon::FD>&, uint32_t);
#else
extern "C" const ctt::CurveOps* ctt_ops_banderwagon(void) { return ctt::CurveImpl<ctt::Banderwagon>::ops(); }
#endif
