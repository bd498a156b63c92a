// The build-time check of sim_jit.h: the header that the library compiles at run time in front of a user's simulator kind,
// instantiated here with the two example kinds of rlrep_amd/envs/kinds/ under the ordinary build, with the run-time compile's -ffp-contract=off
// (build.sh).  The six kernels are launched by nobody: they exist so that a change to sim_jit.h or to an example that does not compile, spills
// or needs LDS shows in the build and in the library's disassembly.
#include "sim_jit.h"
#include "pendulum.h"
#include "point_mass.h"
RL_SIMX_KERNELS(KindPendulum, check_pendulum)
RL_SIMX_KERNELS(KindPointMass, check_point_mass)
