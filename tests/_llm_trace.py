"""Helpers shared by the LLM logit-trace tests (CPU: test_llm_oracle_modes_cpu.py, GPU: test_llm_logits_gpu.py)."""
import json
import os

import torch

from _bars import _OUT          # the directory bar() records into: the raw distances go next to bars.jsonl


def dist(got, ref):
    """(max, rms) over the vocabulary of |got - ref| per step, relative to that step's max |ref|; got, ref: [steps, vocab].
    Returns two float64 tensors [steps]."""
    got, ref = got.double(), ref.double()
    scale = ref.abs().amax(dim=-1)
    d = got - ref
    return d.abs().amax(dim=-1) / scale, d.pow(2).mean(dim=-1).sqrt() / scale


def record(name, **vals):
    """Raw distances next to bars.jsonl (the bars hold ratios; these are what the ratios were made of)."""
    try:
        os.makedirs(_OUT, exist_ok=True)
        with open(os.path.join(_OUT, 'llm_logit_distances.jsonl'), 'a') as f:
            f.write(json.dumps(dict(case=name, **vals)) + '\n')
    except OSError:
        pass


def oracle_traces(sdr, sd64, lm_input, ids):
    """fp64, split-operand and fp32 traces of one teacher-forced sequence: three [1 + len(ids), vocab] tensors."""
    from oracle import llm as OL
    x = lm_input.detach().cpu().float()
    ref = OL.logit_trace(sd64, x, ids)
    with OL.split_operands():
        mod = OL.logit_trace(sdr, x, ids)
    return ref, mod, OL.logit_trace(sdr, x, ids)
