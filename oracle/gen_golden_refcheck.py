"""TEST INFRASTRUCTURE ONLY -- tests/golden/refcheck.npz: the REFERENCE's own outputs for two checks that once ran the reference in place.

Build container only (needs the reference, oracle/ref_harness.py):  python -m oracle.gen_golden_refcheck

* `layer_*`: the `tiny` case of oracle/gen_golden.py, VTG rows [1, 4] -- the reference's prepare_inputs_labels_for_multimodal (attention mask, CPN mask,
  spliced embeddings, labels) and its decoder's final hidden states (tests/test_oracle_golden.py::test_reference_importable_and_agrees_on_one_layer).
* `pre_<k>`: the reference's UMTImageProcessor on random uint8 frames (numpy RandomState(5), the shapes of PREPROCESS_CASES), fp16 pixel values
  (tests/test_vision_oracle.py::test_preprocess_matches_the_reference_image_processor).
* `score_*` / `cpn_*`: the reference's training_utils.calculate_score / calculate_cpn_score on the matrices of coefficient_inputs() -- the two ensembled
  matrices and the two chosen coefficients of each (tests/test_host_logic.py::test_coefficient_sweeps_match_the_reference_when_present).
Inputs are regenerated from their seeds; only the reference's outputs are stored.
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from blim_amd import synth  # noqa: E402
from oracle import blim_oracle as O  # noqa: E402
from oracle.gen_golden import CASES  # noqa: E402

LAYER_ROWS = [1, 4]
PREPROCESS_SEED = 5
PREPROCESS_CASES = (((3, 48, 64, 3), 32), ((2, 32, 32, 3), 32), ((2, 100, 75, 3), 64))     # (frames shape, output size)


def preprocess_frames():
    rs = np.random.RandomState(PREPROCESS_SEED)
    return [(rs.randint(0, 256, size=shape, dtype=np.uint8), S) for shape, S in PREPROCESS_CASES]


def coefficient_inputs():
    """Four 40 x 40 similarity matrices (t2v / v2t of the two stages) and the identity id maps the coefficient sweeps take."""
    rs = np.random.RandomState(4)
    n = 40
    a, b = rs.randn(n, n).astype(np.float32) + 1.5 * np.eye(n, dtype=np.float32), rs.randn(n, n).astype(np.float32) + 0.5 * np.eye(n, dtype=np.float32)
    c, d = rs.randn(n, n).astype(np.float32) + 1.0 * np.eye(n, dtype=np.float32), rs.randn(n, n).astype(np.float32)
    ids = {i: i for i in range(n)}
    return a, b, c, d, ids


def layer_inputs():
    """The tiny case's oracle model, problem and padded VTG rows (what tests/test_oracle_golden.py's `tiny` fixture builds)."""
    spec = CASES["tiny"]
    dims = synth.ModelDims(**spec["dims"])
    cfg = O.OracleConfig(**spec["dims"])
    w = O.synthetic_weights(cfg, spec["wseed"])
    prob = synth.make_problem(spec["pseed"], spec["n"], dims, tok_per_clip=spec["tok_per_clip"], text_len=spec["text_len"])
    vtg = O.padding_ids(prob.vtg_ids, prob.vtg_labels, prob.vtg_masks, synth.PAD_ID)
    return cfg, w, prob, vtg


def main():
    import torch
    from oracle import ref_harness
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "refcheck.npz"))
    a = ap.parse_args()
    if not ref_harness.available():
        sys.exit("reference not present; fixtures can only be generated in the build container")
    out = {}
    cfg, w, prob, (ids, lab, msk) = layer_inputs()
    ref = ref_harness.build_model(cfg, w)
    sel = LAYER_ROWS
    T = lambda x: torch.from_numpy(np.asarray(x))
    with torch.no_grad():
        r = ref.prepare_inputs_labels_for_multimodal(T(ids[sel]), None, T(msk[sel]), None, T(lab[sel]), [T(prob.video[i]) for i in sel],
                                                     ["video"] * len(sel), image_sizes=None, video_feature=True, cpn=True)
        (_, _, (m_r, c_r), _, e_r, l_r) = r
        h_r = ref(inputs_embeds=e_r, attention_mask=m_r).hidden_states
    out.update(layer_mask=m_r.numpy(), layer_cpn=c_r.numpy(), layer_embeds=e_r.numpy().astype(np.float32), layer_labels=l_r.numpy(),
               layer_hidden=h_r.numpy().astype(np.float32))
    ref_harness.load()
    from videochat_flash.vision_tower_builder import UMTImageProcessor
    for k, (frames, S) in enumerate(preprocess_frames()):
        out[f"pre_{k}"] = UMTImageProcessor(size=(S, S)).preprocess(frames, return_tensors="pt")["pixel_values"].half().numpy()
    R = ref_harness.load().TU
    a_, b_, c_, d_, ids = coefficient_inputs()
    for tag, fn in (("score", R.calculate_score), ("cpn", R.calculate_cpn_score)):
        m0, m1, k0, k1 = fn(a_, b_, c_, d_, ids, ids)
        out.update({f"{tag}_m0": np.asarray(m0), f"{tag}_m1": np.asarray(m1), f"{tag}_coef": np.array([k0, k1], dtype=np.float64)})
    np.savez_compressed(a.out, **out)
    print(f"wrote {a.out} ({os.path.getsize(a.out) / 1e6:.2f} MB): " + ", ".join(f"{k} {v.shape} {v.dtype}" for k, v in out.items()))


if __name__ == "__main__":
    main()
