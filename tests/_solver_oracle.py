"""The CPU oracle's flow inference under solver settings, shared by tests/golden/make_golden_solver.py and the solver tests.
oracle.flow.inference takes the step count; the guidance rate is an argument of oracle.flow.solve_euler only, which inference looks up at
call time -- so it is wrapped for the duration of the call and oracle/ itself is not touched."""
import torch

SETTINGS = ((1, 0.7), (4, 0.7), (16, 0.7), (10, 0.0), (10, 1.5))          # (steps, cfg_rate) of tests/golden/flow_solver.npz
TAGS = (('full', False, True), ('stream_nonfinal', True, False))          # tag, streaming, finalize


def key(tag, steps, cfg):
    return f'mel_{tag}_n{steps}_c{cfg:g}'


def inference(sd, token, prompt_token, prompt_feat, embedding, streaming, finalize, steps, cfg):
    from oracle import flow as OF
    real = OF.solve_euler

    def solve(sd_, z, mu, mask, spks, cond, n_timesteps=10, streaming=False, **kw):
        return real(sd_, z, mu, mask, spks, cond, n_timesteps, streaming, cfg=cfg, **kw)
    OF.solve_euler = solve
    try:
        with torch.inference_mode():
            return OF.inference(sd, token, prompt_token, prompt_feat, embedding, streaming, finalize, n_timesteps=steps)
    finally:
        OF.solve_euler = real


def walk(span):
    """t and dt of every Euler step as solve_euler walks a t_span (flow_matching.py:91-121), in fp32 torch arithmetic"""
    t, dt = span[0:1].clone(), span[1] - span[0]
    ts, dts = [], []
    for step in range(1, len(span)):
        ts.append(t.clone())
        dts.append(dt.clone().reshape(1))
        t = t + dt
        if step < len(span) - 1:
            dt = span[step + 1] - t
    return torch.cat(ts), torch.cat(dts)
