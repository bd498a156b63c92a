// A point mass in the plane as a fused-simulator kind given as text (csrc/sim_jit.h; CustomFusedSim); the host twin is
// rlrep_amd/envs/point_mass.py, operation for operation.  x = (px, py, vx, vy), fp64; the observation is x rounded to fp32; two actions, the
// force, clipped to +-1 per component.  One step, semi-implicit Euler with dt = 0.1:
//     v <- clamp(v + f dt, +-1)        p <- clamp(p + v dt, +-2)        (per component; the walls are inelastic only in position)
//     d = sqrt(px^2 + py^2)            goal = d < 0.1                   r = (-d - 0.01 (fx^2 + fy^2)) + (goal ? 10 : 0)
// The goal ends the episode; the time limit is 100 steps.  Start: px ~ U(-1, 1) from words 0, 1 of Philox block 0, py ~ U(-1, 1) from words
// 0, 1 of block 1 (c[4], c[5]), speed 0.  Only + - * /, compares and sqrt: a NumPy float64 restatement reproduces every bit.
struct KindPointMass {
    static constexpr int NX = 4, S = 4, A = 2, LIMIT = 100;
    static constexpr bool TERMINATES = true;
    static constexpr float ACT_LO = -1.0f, ACT_HI = 1.0f;
    static __device__ __forceinline__ double clamp(double v, double lo, double hi) { return v < lo ? lo : (v > hi ? hi : v); }
    static __device__ __forceinline__ void start(const uint32_t* c, double* x) {
        x[0] = -1.0 + 2.0 * simx_u01d(c[0], c[1]);
        x[1] = -1.0 + 2.0 * simx_u01d(c[4], c[5]);
        x[2] = 0.0; x[3] = 0.0;
    }
    static __device__ __forceinline__ void observe(const double* x, float* obs) {
        obs[0] = (float)x[0]; obs[1] = (float)x[1]; obs[2] = (float)x[2]; obs[3] = (float)x[3];
    }
    static __device__ __forceinline__ float dynamics(double* x, const float* a, bool& goal) {
        const double fx = clamp((double)a[0], -1.0, 1.0), fy = clamp((double)a[1], -1.0, 1.0);
        const double vx = clamp(x[2] + fx * 0.1, -1.0, 1.0), vy = clamp(x[3] + fy * 0.1, -1.0, 1.0);
        const double px = clamp(x[0] + vx * 0.1, -2.0, 2.0), py = clamp(x[1] + vy * 0.1, -2.0, 2.0);
        const double d = sqrt(px * px + py * py);
        goal = d < 0.1;
        const double r = (-d - 0.01 * (fx * fx + fy * fy)) + (goal ? 10.0 : 0.0);
        x[0] = px; x[1] = py; x[2] = vx; x[3] = vy;
        return (float)r;
    }
};
