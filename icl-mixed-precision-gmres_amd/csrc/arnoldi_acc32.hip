// fp32-accumulation build of the fused Arnoldi phases (mpg_arnoldi_set_accum,
// include/mpgmres/arnoldi.h): the launch code of arnoldi_launch.hpp with A =
// float, for the fp32-Arnoldi type combinations (single, mixed, mixed-half).
// Its own translation unit, so it compiles beside arnoldi.hip.
#include "arnoldi_launch.hpp"

const mpg_arnoldi_phases& mpg_arnoldi_phases_acc32() {
    static const mpg_arnoldi_phases table = phases_of<float>();
    return table;
}
