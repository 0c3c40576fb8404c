// nmf_tree_fwd.h — declarations of what the stage headers call of nmf_tree.h (the sweeps of the rest of the body / of a general
// tree).  nmf_tree.h itself has to come last in the stepping kernel's translation unit: its articulated-body passes are built
// from aba_step / add_contact_K_row of nmf_step_aba.h, whose aba_solve in turn calls them.
#pragma once
#include "nmf_step_lds.h"

namespace nmf {

struct RestNode;
struct InertiaRowMap;

// kinematics, velocities and bias accelerations
template <class TP> __device__ void tree_kinematics_chain(FlyLds<TP>& s, const GModel& m, int lane, float (*relm)[12]);
template <class TP> __device__ void tree_velocity_bias(FlyLds<TP>& s, const GModel& m, int lane);
// twists, projections, the articulated-body solve of a general tree
template <class TP> __device__ void tree_sweep_twists(FlyLds<TP>& s, const float* x, float (*T)[row_width_tw<TP>()], const GModel& m, int lane);
template <class TP, class Extra, class Emit>
__device__ __forceinline__ void tree_sweep_project(FlyLds<TP>& s, float (*W)[row_width_tw<TP>()], const GModel& m, int lane, Extra&& extra, Emit&& emit);
template <class TP, bool WELD>
__device__ void tree_aba_solve(FlyLds<TP>& s, int tau_id, int x_id, bool withK, float hdamp, const GModel& m, int lane);
// the rest of the body below a star kernel's root
template <class TP> __device__ void tree_sweep_twists_levels(FlyLds<TP>& s, const float* x, float (*T)[row_width_tw<TP>()], const GModel& m, int lane);
template <class TP, class Extra>
__device__ __forceinline__ void tree_gather_levels(FlyLds<TP>& s, float (*W)[row_width_tw<TP>()], const GModel& m, int lane, Extra&& extra);
template <class TP, bool FAST, bool UP, bool LANE_PER_BODY = false, class F>
__device__ __forceinline__ void rest_levels(FlyLds<TP>& s, int lane, F&& f);
template <class TP, int NUM>
__device__ __forceinline__ void rest_aba_eliminate(FlyLds<TP>& s, const RestNode& nd, const float* tau, bool withK, float hdamp,
                                                   const Frame& fr, const LaneRole& L, const int (&so)[6], const InertiaRowMap& IM, const GModel& m);
template <class TP, int NUM, bool HOMOGENEOUS>
__device__ __forceinline__ void rest_aba_expand(FlyLds<TP>& s, const RestNode& nd, float* x, const LaneRole& L);

}  // namespace nmf
