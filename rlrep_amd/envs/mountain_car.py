"""NumPy MountainCarContinuous-v0 with the pre-0.26 gym API the launcher uses (`env.seed`, `reset() -> obs`,
`step() -> (obs, reward, done, info)`, `env._max_episode_steps`), in the style of envs/pendulum.py.

Dynamics are the public gym specification: action clipped to +-1, power 0.0015, velocity clipped to +-0.07, position to [-1.2, 0.6], an
inelastic left wall, the goal `position >= 0.45 and velocity >= 0` ends the episode with +100, reward -0.1 a^2 of the RAW action, 999-step
time limit, reset position ~ U(-0.6, -0.4) at rest.  Nothing here comes from the reference repository.

Arithmetic is fp64; the state is HELD as the fp32 values the observation shows (gym keeps it in a float32 array): position and velocity are
rounded to fp32 at reset and at the end of every step, and the goal is decided on the fp64 values before that rounding.  So an observation
determines the state exactly, and the device kernel (csrc/group_env.h EnvMountainCar) restates step() operation for operation.
"""
import numpy as np

from .pendulum import Box


class MountainCarContinuousEnv:
    min_action, max_action = -1.0, 1.0
    min_position, max_position, max_speed = -1.2, 0.6, 0.07
    goal_position, goal_velocity, power = 0.45, 0.0, 0.0015
    _max_episode_steps = 999

    def __init__(self, seed=None):
        self._rng = np.random.RandomState(seed)
        self.action_space = Box([self.min_action], [self.max_action], self._rng)
        self.observation_space = Box([self.min_position, -self.max_speed], [self.max_position, self.max_speed], self._rng)
        self._t = 0
        self._p, self._v = float(np.float32(-0.5)), 0.0
        self._unrounded = (self._p, self._v)

    def seed(self, seed=None):
        self._rng.seed(seed)
        return [seed]

    def _obs(self):
        return np.array([self._p, self._v], np.float32)

    def reset(self):
        self._p = float(np.float32(self._rng.uniform(-0.6, -0.4)))
        self._v = 0.0
        self._t = 0
        return self._obs()

    def step(self, action):
        a = float(np.asarray(action).reshape(-1)[0])
        force = min(max(a, self.min_action), self.max_action)
        p, v = self._p, self._v
        v = v + (force * self.power - 0.0025 * float(np.cos(3.0 * p)))
        v = min(max(v, -self.max_speed), self.max_speed)
        p = p + v
        p = min(max(p, self.min_position), self.max_position)
        if p == self.min_position and v < 0.0:
            v = 0.0
        goal = p >= self.goal_position and v >= self.goal_velocity
        reward = (100.0 if goal else 0.0) - 0.1 * (a * a)
        self._unrounded = (p, v)                # what `goal` was decided on
        self._p, self._v = float(np.float32(p)), float(np.float32(v))
        self._t += 1
        return self._obs(), reward, bool(goal or self._t >= self._max_episode_steps), {}
