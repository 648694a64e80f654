"""Fixture of the fp16 flow engine's chain test (tests/test_flow_fp16_gpu.py): chain_rounded_f16.npz, the mel of fullsize.npz's tokens from the
ORACLE flow with every matrix-product operand rounded to fp16 -- round to nearest even, saturated to +-65504, where the fp16 HIP path rounds --
and everything else fp32.  What fp16 operand rounding alone does in the reference's arithmetic: make_golden.py's gen_chain_rounded with the
oracle's bf16 operand rounding (oracle.flow._r) replaced at run time; oracle/ itself is not touched (_linear, _conv1d and _matmul look _r up
at call time).  ~100 s of CPU:  python tests/golden/make_golden_fp16.py"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'cosyvoice2-eu_amd'))

from cv2amd import synth            # noqa: E402
from oracle import flow as OF       # noqa: E402


def r_f16(x):
    """oracle.flow._r with fp16 in place of bf16."""
    return x.clamp(-65504.0, 65504.0).half().float() if OF.ROUND['on'] else x


def gen_chain_rounded_f16():
    gd = np.load(os.path.join(HERE, 'fullsize.npz'))
    inp = synth.synthetic_inputs(prompt_len=int(gd['prompt_len']))
    fsd = synth.make_flow()
    bf16_r = OF._r
    OF._r = r_f16
    try:
        with torch.inference_mode(), OF.rounded_operands():
            mr = OF.inference(fsd, torch.from_numpy(gd['token']), inp['prompt_token'], inp['prompt_feat'], inp['embedding'], False, True)
    finally:
        OF._r = bf16_r
    np.savez_compressed(os.path.join(HERE, 'chain_rounded_f16.npz'), mel_rounded=mr[0].numpy().astype(np.float32))


if __name__ == '__main__':
    gen_chain_rounded_f16()
