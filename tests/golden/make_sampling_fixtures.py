"""Writes tests/golden/sampling_kats.npz: the answers of tests/llm_sampling_ref.py (the numpy float64 statement of
astts_op_sample_topk_topp) on its CASES -- per case the drawn tokens for the case's fixed uniforms, the nucleus ids in order and their
renormalised probabilities q (float32).  The inputs regenerate from numpy.random.default_rng(seed); only the answers are stored (kilobytes).
A case whose smallest margin is below MARGIN is refused: pick another seed in CASES.

    python tests/golden/make_sampling_fixtures.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import llm_sampling_ref as ref  # noqa: E402


def build():
    out = {}
    for case in ref.CASES:
        tokens, margin, rows = ref.case_answers(case)
        assert margin >= ref.MARGIN, f"{case[0]}: margin {margin:.2e} < {ref.MARGIN}: choose another seed"
        width = max(len(r.ids) for r in rows)
        out[case[0] + "/tokens"] = tokens.astype(np.int32)
        out[case[0] + "/sizes"] = np.array([len(r.ids) for r in rows], np.int32)          # ids and q: the rows' nuclei one after another
        out[case[0] + "/ids"] = np.concatenate([r.ids for r in rows]).astype(np.int32)
        out[case[0] + "/q"] = np.concatenate([r.q for r in rows]).astype(np.float32)
        print(f"{case[0]}: nucleus sizes {min(len(r.ids) for r in rows)} .. {width}, smallest margins kth {min(r.kth for r in rows):.2e} "
              f"nucleus {min(r.nucleus for r in rows):.2e} draw {min(r.draw for r in rows):.2e}")
    return out


if __name__ == "__main__":
    np.savez_compressed(os.path.join(HERE, "sampling_kats.npz"), **build())
