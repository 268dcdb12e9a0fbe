// stack_linfit.hip -- register-resident StackLinearFit for gfx950, BIT-EXACT: the default pass's instantiations of the
// kernels in stack_linfit_impl.hpp (which has the method and the exactness argument) and their launchers.
#include "stack_linfit_impl.hpp"

namespace nl {

int linfit_ml_supported(int mode, int n_frames, int64_t npix)
{
    return (mode == NL_ST_LINEAR_FIT && n_frames > 128 && n_frames <= 512 && npix < kFastMaxPixels) ? 1 : 0;
}

int linfit_fast_supported(int mode, int n_frames, int64_t npix)
{
    return (mode == NL_ST_LINEAR_FIT && n_frames >= 1 && n_frames <= 128 && npix < kFastMaxPixels) ? 1 : 0;
}

// (stack_linfit_maps.hip: the MAPS instantiations)
hipError_t launch_linfit_ml_maps(const StackArgs &args, const FastArgs &fargs, const LinfitCascade *cascade,
                                 hipStream_t stream, const char **name, hipEvent_t dominant_done);
hipError_t launch_linfit_fast_maps(const StackArgs &args, const FastArgs &fargs, const LinfitCascade *cascade,
                                   hipStream_t stream, const char **name, hipEvent_t dominant_done);

hipError_t launch_stack_linfit_ml(const StackArgs &args, const FastArgs &fargs, const LinfitCascade *cascade,
                                  hipStream_t stream, const char **name, hipEvent_t dominant_done, Form form)
{
    if ((form != Form::Plain && form != Form::Maps) || !form_args_ok(form, args)) return hipErrorInvalidValue;
    return form == Form::Maps ? launch_linfit_ml_maps(args, fargs, cascade, stream, name, dominant_done)
                              : launch_linfit_ml<false>(args, fargs, cascade, stream, name, dominant_done);
}

hipError_t launch_stack_linfit_fast(const StackArgs &args, const FastArgs &fargs, const LinfitCascade *cascade,
                                    hipStream_t stream, const char **name, hipEvent_t dominant_done, Form form)
{
    if ((form != Form::Plain && form != Form::Maps) || !form_args_ok(form, args)) return hipErrorInvalidValue;
    return form == Form::Maps ? launch_linfit_fast_maps(args, fargs, cascade, stream, name, dominant_done)
                              : launch_linfit_fast<false>(args, fargs, cascade, stream, name, dominant_done);
}

}  // namespace nl
