// Pendulum-v1 as a fused-simulator kind given as text (csrc/sim_jit.h; CustomFusedSim): the operations of csrc/group_env.h EnvPendulum,
// i.e. of rlrep_amd/envs/pendulum.py -- g = 10, m = l = 1, dt = 0.05, torque clipped to +-2, speed to +-8, reward from the wrapped angle, a
// 200-step time limit and no other end, reset theta ~ U(-pi, pi), theta_dot ~ U(-1, 1).  x = (theta, theta_dot), fp64.
struct KindPendulum {
    static constexpr int NX = 2, S = 3, A = 1, LIMIT = 200;
    static constexpr bool TERMINATES = false;
    static constexpr float ACT_LO = -2.0f, ACT_HI = 2.0f;
    static __device__ __forceinline__ void start(const uint32_t* c, double* x) {
        x[0] = -SIMX_PI + 2.0 * SIMX_PI * simx_u01d(c[0], c[1]);
        x[1] = -1.0 + 2.0 * simx_u01d(c[2], c[3]);
    }
    static __device__ __forceinline__ void observe(const double* x, float* obs) {
        obs[0] = (float)cos(x[0]); obs[1] = (float)sin(x[0]); obs[2] = (float)x[1];
    }
    static __device__ __forceinline__ float dynamics(double* x, const float* a, bool& goal) {
        const double th = x[0], thd = x[1];
        const double u = fmin(fmax((double)a[0], -2.0), 2.0);
        double wrapped = fmod(th + SIMX_PI, 2.0 * SIMX_PI);             // Python's float %: the sign of the divisor
        if (wrapped < 0.0) wrapped += 2.0 * SIMX_PI;
        wrapped -= SIMX_PI;
        const double cost = (wrapped * wrapped + 0.1 * (thd * thd)) + 0.001 * (u * u);
        double v = thd + (15.0 * sin(th) + 3.0 * u) * 0.05;
        v = fmin(fmax(v, -8.0), 8.0);
        x[0] = th + v * 0.05;
        x[1] = v;
        goal = false;
        return (float)(-cost);
    }
};
