"""Flow solver settings of ONE call (an extension: the reference passes `n_timesteps` to CausalConditionalCFM.forward and reads the attribute
`inference_cfg_rate` inside solve_euler, flow_matching.py:71-123; conf/cosyvoice2.yaml fixes 10 steps and rate 0.7 per model).

A `Solver` value travels with a call from the public surface (CosyVoice2.solver(...)) to every flow invocation of the call.  Its device form
is the utterance's cv2_flow_solver record (include/cv2_amd.h): `steps` Euler steps on the cosine grid 1 - cos(linspace(0, 1, steps + 1) * pi / 2)
and the guidance rate of the update x + dt * ((1 + cfg_rate) * v_cond - cfg_rate * v_uncond).  Utterances with different rates share a launch;
one launch has one step count, so the engine and the scheduler group calls by it.  Pure Python: the CPU tests import it without a device.
"""
import math

from .sampling import f32

FIELDS = ('steps', 'cfg_rate')
F32_MAX = 3.4028234663852886e38       # the device holds the rate as a float
MAX_STEPS = 31                         # include/cv2_amd.h: the time tables hold 1 .. 31 steps


class Solver:
    """steps, cfg_rate: None = the engine's (cv2amd/config.py: n_timesteps, inference_cfg_rate of conf/cosyvoice2.yaml)."""
    __slots__ = FIELDS

    def __init__(self, steps=None, cfg_rate=None):
        self.steps, self.cfg_rate = steps, cfg_rate

    def __repr__(self):
        return 'Solver(' + ', '.join(f'{k}={getattr(self, k)!r}' for k in FIELDS if getattr(self, k) is not None) + ')'

    def __eq__(self, o):
        return isinstance(o, Solver) and all(getattr(self, k) == getattr(o, k) for k in FIELDS)

    def __hash__(self):
        return hash((self.steps, self.cfg_rate))

    def is_default(self):
        """nothing set: no record is written and the call takes the path of a call without settings"""
        return self.steps is None and self.cfg_rate is None

    def replace(self, **kw):
        """a copy with the given (non-None) fields replaced"""
        d = {k: getattr(self, k) for k in FIELDS}
        d.update({k: v for k, v in kw.items() if v is not None})
        return Solver(**d)

    def check(self):
        """ValueError for anything outside the accepted ranges (before any work); returns self"""
        if self.steps is not None:
            if isinstance(self.steps, bool) or not isinstance(self.steps, int):
                raise ValueError(f'solver: steps must be an integer, got {self.steps!r}')
            if not 1 <= self.steps <= MAX_STEPS:
                raise ValueError(f'solver: steps {self.steps} outside 1 .. {MAX_STEPS}')
        if self.cfg_rate is not None:
            if isinstance(self.cfg_rate, bool) or not isinstance(self.cfg_rate, (int, float)) or not math.isfinite(self.cfg_rate):
                raise ValueError(f'solver: cfg_rate must be a finite number, got {self.cfg_rate!r}')
            if not 0 <= self.cfg_rate <= F32_MAX:
                raise ValueError(f'solver: cfg_rate {self.cfg_rate} outside 0 .. 3.4e38')
        return self

    def resolve(self, engine):
        """(steps, cfg_rate) the call runs under: unset fields from `engine` (anything with n_timesteps and cfg_rate, a FlowEngine), the
        rate rounded to float32 as the device holds it.  Two settings that resolve to equal pairs are the same computation."""
        steps = int(engine.n_timesteps) if self.steps is None else self.steps
        rate = engine.cfg_rate if self.cfg_rate is None else self.cfg_rate
        return steps, f32(float(rate))


def resolve(solver, engine):
    """resolve() of a setting that may be None"""
    return (solver or Solver()).resolve(engine)
