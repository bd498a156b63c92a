"""Minimal environments so that BASELINE config (1) (sac on Pendulum-v1) runs with no gym/MuJoCo installed; MountainCarContinuous-v0 beside it."""
from .pendulum import PendulumEnv, make  # noqa: F401
from .mountain_car import MountainCarContinuousEnv  # noqa: F401
