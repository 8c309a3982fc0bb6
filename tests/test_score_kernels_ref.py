"""CPU: oracle/score_kernels_ref.py, the float64 reference of tests/test_score_kernels_gpu.py, checked without a GPU.

1. Every reference agrees with an independent plain statement of the operation to 1e-12: torch float64 x * rsqrt(mean(x^2) + eps) * w, a log_softmax written out in
   numpy float64, gemm_ref.lse_combine, plain means and copies.
2. A plain f32 evaluation of each operation in numpy (f32 sums and products, numpy's own exp / log / sqrt) stays inside the tolerance on exactly the inputs the
   GPU tests use (tests/score_kernel_inputs.py): the bounds are not too tight for an honest f32 kernel.
3. Each wrong rule of S.RULES leaves TEN TIMES the tolerance, on the elements it touches, on AT LEAST ONE case of the input set (printed as SCORE_KERNEL_RULE lines,
   case by case).  Not on every case: a rule about the gather needs a gather, one about saturation fp16 and the `massive` family.
4. The exact checks of the GPU tests -- hi / lo bit-identity, tile bytes, sentinels, assemble bytes -- are fed a variant's bytes and must fail."""
import numpy as np
import pytest
import torch

import score_kernel_inputs as I
from oracle import gemm_ref as G
from oracle import score_kernels_ref as S
from oracle.attention_ref import bits16, from_bits16, round16

f32 = np.float32
quiet = dict(over="ignore", invalid="ignore", divide="ignore")


def log_softmax(x):
    x = np.asarray(x, np.float64)
    z = x - x.max(-1, keepdims=True)
    return z - np.log(np.exp(z).sum(-1, keepdims=True))


def caught(kernel, rule, figures):
    """figures: (case, ratio of the wrong variant) -- prints them and asserts that one is beyond ten times the tolerance."""
    for case, r in figures:
        print(f"SCORE_KERNEL_RULE kernel={kernel} rule={rule} case={case} ratio={r:.4g}")
    assert figures and max(r for _, r in figures) > 10.0, (kernel, rule, "no case of the input set tells this rule from the right one")


# ---------------------------------------------------------------------------- 1. pins
def test_rmsnorm_is_the_plain_statement():
    rs = np.random.RandomState(3)
    x, w = rs.standard_normal((6, 40)).astype(f32), (1 + 0.2 * rs.standard_normal(40)).astype(f32)
    tx = torch.from_numpy(x.astype(np.float64))
    want = tx * torch.rsqrt((tx * tx).mean(1, keepdim=True) + float(f32(1e-6))) * torch.from_numpy(w.astype(np.float64))
    rows = np.array([5, 0, 0, 3])
    for form in ("narrow4", "narrow16", "wide"):
        np.testing.assert_allclose(S.rmsnorm(x, w, 1e-6, 40, form=form).o, want.numpy(), rtol=1e-12)
        np.testing.assert_allclose(S.rmsnorm(x, w, 1e-6, 40, rows=rows, n_src=6, form=form).o, want.numpy()[rows], rtol=1e-12)
    r = S.rmsnorm(x, w, 1e-6, 40, rows=np.array([1, -1, 6, 2]), n_src=6)
    assert (r.poison == [False, True, True, False]).all() and np.isnan(r.o[1:3]).all() and np.isfinite(r.o[[0, 3]]).all() and (r.tol[1:3] == 0).all()
    assert S.rmsnorm_form(256, 256, 0) == "narrow4" and S.rmsnorm_form(260, 260, 0) == "narrow4" and S.rmsnorm_form(264, 264, 0) == "wide"
    assert S.rmsnorm_form(1028, 1028, 0) == "narrow16" and S.rmsnorm_form(4096, 4096, 4100) == "narrow16" and S.rmsnorm_form(4096, 4096, 8192) == "wide"
    assert S.rmsnorm_form(4100, 4100, 0) is None and S.rmsnorm_form(1024, 1024, 1028) == "narrow4"


def test_rmsnorm_states_the_non_finite_rows():
    c = I.rms((1028, 5, 0, "2H", "hlf", 0, "nonfinite", 1))
    o = c.ref.o
    assert np.isnan(o[0]).all()                                                     # a NaN in the row: ss is NaN
    assert np.isnan(o[1, c.H - 2]) and (np.delete(o[1], c.H - 2) == 0).all()        # an inf: inv = 0, 0 * inf at the inf itself
    assert np.isfinite(o[2:]).all() and (c.ref.tol[:2] == 0).all() and (c.ref.tol[2:] > 0).all()


def test_split16_rule():
    o = np.array([[1.0 + 2.0 ** -12, 7.0e4, -1.0e6, np.inf, np.nan, 1e-9, -0.0]], f32)
    hi, lo = S.split16(o, "f16", saturate=True)
    assert hi[0, 0] == 1.0 and lo[0, 0] == 2.0 ** -12
    assert hi[0, 1] == 65504.0 and lo[0, 1] == 7.0e4 - 65504.0                      # lo continues from the SATURATED hi
    assert hi[0, 2] == -65504.0 and lo[0, 2] == -65504.0                            # ... and saturates itself
    assert hi[0, 3] == np.inf and np.isnan(lo[0, 3]) and np.isnan(hi[0, 4]) and np.isnan(lo[0, 4])
    assert hi[0, 5] == 0.0 and lo[0, 5] == 0.0 and np.signbit(hi[0, 6])
    hi, lo = S.split16(o, "f16", saturate=False)
    assert hi[0, 1] == np.inf and lo[0, 1] == -np.inf
    hi, lo = S.split16(o, "bf16")
    assert hi[0, 1] == round16(7.0e4, "bf16") and lo[0, 1] == round16(7.0e4 - hi[0, 1], "bf16")
    hi, lo = S.split16(o, "f16", poison=np.array([True]))
    assert np.isnan(hi).all() and (lo == 0).all()


def test_criteria_are_log_softmax():
    c = I.ce((257, 5, 3, "masked"))
    want = np.where(c.labels < 0, 0.0, log_softmax(c.buf[:, :c.V])[np.arange(c.n), np.maximum(c.labels, 0)])
    np.testing.assert_allclose(c.ref, want, rtol=1e-12, atol=1e-13)
    assert c.ref[1] == 0.0 and c.tol[1] == 0.0
    c = I.tvg((5, 65, 3, 3))
    ls = log_softmax(c.buf[:, :c.nv]).reshape(c.n_pairs, c.clips, c.nv)
    np.testing.assert_allclose(c.ref, ls[np.arange(c.n_pairs), :, c.labels].mean(1), rtol=1e-12)
    c = I.lse((594, 9, "masked"))
    want = np.where(c.labels < 0, 0.0, c.ll.astype(np.float64) - G.lse_combine(c.m, c.s))
    np.testing.assert_allclose(c.ref, want, rtol=1e-12)
    c = I.lse((65, 5, "empty_tiles"))
    x = [np.concatenate([mm + np.log(ss / 4.0) * np.ones(4) for mm, ss in zip(m.astype(np.float64), s.astype(np.float64)) if ss > 0]) for m, s in zip(c.m, c.s)]
    want = np.array([ll - (xx.max() + np.log(np.exp(xx - xx.max()).sum())) for ll, xx in zip(c.ll.astype(np.float64), x)])        # tiles rebuilt as four equal logits each
    np.testing.assert_allclose(c.ref, want, rtol=1e-12)


def test_segment_mean_pins_the_zero_counts():
    c = I.seg((129, 0))
    lp, rs = c.lp.astype(np.float64), c.row_start
    assert rs[3] == rs[2] and (lp[rs[3]:rs[4]] == 0).all() and rs[4] - rs[3] == 5
    assert np.isnan(c.ref[2]) and np.isnan(c.ref[3])                                 # mode 0: sum / count_nonzero -- an empty and an all-zero segment are 0 / 0
    ok = np.isfinite(c.ref)
    assert ok.sum() == 127
    np.testing.assert_allclose(c.ref[ok], [lp[rs[p]:rs[p + 1]].sum() / np.count_nonzero(lp[rs[p]:rs[p + 1]]) for p in np.flatnonzero(ok)], rtol=1e-12)
    c1 = I.seg((129, 1))
    assert np.isnan(c1.ref[2]) and c1.ref[3] == 0.0 and np.isfinite(np.delete(c1.ref, 2)).all()      # mode 1: only the empty segment
    np.testing.assert_allclose(c1.ref[1], lp[rs[1]:rs[2]].mean(), rtol=1e-12)
    assert any((lp[rs[p]:rs[p + 1]] == 0).any() and (lp[rs[p]:rs[p + 1]] != 0).any() for p in range(129))


def test_group_mean_and_assemble_are_the_plain_statements():
    c = I.gm((3, 5, 8, 1), "f16")
    want = (c.x[:, :8] + c.x[:, 8:]).reshape(5, 3, 8).mean(1)
    np.testing.assert_allclose(c.ref.mean, want, rtol=1e-12)
    assert (c.x[:, 8:] != 0).any() and (c.ref.hi_lo <= round16(want, "f16")).all() and (round16(want, "f16") <= c.ref.hi_hi).all()
    c = I.gm((64, 5, 1024, 0), "bf16")
    np.testing.assert_allclose(c.ref.mean, c.x.reshape(5, 64, 1024).mean(1), rtol=1e-12)
    c = I.asm((8, 1))
    assert (c.ref[0, :8] == c.table[0]).all() and (c.ref[0, 8:] == 0).all() and (c.ref[1] == c.feats[0]).all() and (c.ref[3] == c.feats[3]).all()
    assert (c.ref[2, :8] == c.table[5]).all() and (I.asm((8, 0)).ref[3] == I.asm((8, 0)).feats[3]).all()


def test_rmsnorm_f8_scale_rule():
    c = I.rms_f8((1028, 5, "zero"))
    assert c.ref.scale[0] == 1.0 and c.ref.tol_scale[0] == 0.0
    np.testing.assert_allclose(c.ref.scale[1:], np.abs(c.ref.o[1:]).max(1) / 448.0, rtol=1e-15)
    q = G.e4m3_decode(G.e4m3_encode(c.ref.o / c.ref.scale[:, None])) * c.ref.scale[:, None]          # the ideal quantiser is inside the bound
    assert I.ratio(q, c.ref.o, c.ref.tol_val(c.ref.scale)) <= 0.5


# ---------------------------------------------------------------------------- 2. a plain f32 evaluation is inside the bounds
def _rms_f32(c):
    src = np.arange(c.n) if c.rows is None else c.rows
    o = np.full((c.n, c.H), np.nan, f32)
    with np.errstate(**quiet):
        for i, s in enumerate(src):
            if 0 <= s < c.n_src:
                x = c.x[s]
                inv = f32(1.0) / np.sqrt(f32((x * x).sum(dtype=f32) / f32(c.H) + f32(I.RMS_EPS)))
                o[i] = c.w * (x * inv)
    return o


@pytest.mark.parametrize("case", I.RMS, ids=str)
def test_f32_rmsnorm_is_inside(case):
    c = I.rms(case)
    assert I.ratio(_rms_f32(c), c.ref.o, c.ref.tol) <= 1.0


def test_f32_criteria_are_inside():
    for case in I.CE:
        c = I.ce(case)
        x = c.buf[:, :c.V]
        z = x - x.max(1, keepdims=True)
        got = np.where(c.labels < 0, f32(0), x[np.arange(c.n), np.maximum(c.labels, 0)] - (x.max(1) + np.log(np.exp(z).sum(1, dtype=f32))))
        assert got.dtype == f32 and I.ratio(got, c.ref, c.tol) <= 1.0, case
    for case in I.TVG:
        c = I.tvg(case)
        x = c.buf[:, :c.nv]
        z = x - x.max(1, keepdims=True)
        per = x[np.arange(len(x)), np.repeat(c.labels, c.clips)] - (x.max(1) + np.log(np.exp(z).sum(1, dtype=f32)))
        got = per.reshape(c.n_pairs, c.clips).sum(1, dtype=f32) / f32(c.clips)
        assert got.dtype == f32 and I.ratio(got, c.ref, c.tol) <= 1.0, case
    for case in I.LSE:
        c = I.lse(case)
        with np.errstate(**quiet):
            big = c.m.max(1, keepdims=True)
            e = np.where(c.m > -np.inf, c.s * np.exp(c.m - big), f32(0))
            got = np.where(c.labels < 0, f32(0), c.ll - (big[:, 0] + np.log(e.sum(1, dtype=f32))))
        assert got.dtype == f32 and I.ratio(got, c.ref, c.tol) <= 1.0, case
    for case in I.SEG:
        c = I.seg(case)
        got = np.zeros(c.n_pairs, f32)
        with np.errstate(**quiet):
            for p in range(c.n_pairs):
                sg = c.lp[c.row_start[p]:c.row_start[p + 1]]
                acc = f32(0)
                for v in sg:
                    acc = f32(acc + v)
                got[p] = acc / f32(np.count_nonzero(sg) if c.mode == 0 else len(sg))
        assert I.ratio(got, c.ref, c.tol) <= 1.0, case


@pytest.mark.parametrize("dtype", I.DTYPES)
def test_f32_group_mean_is_inside(dtype):
    for case in I.GM:
        c = I.gm(case, dtype)
        H = c.H
        v = (c.x[:, :H].astype(f32) + c.x[:, H:].astype(f32)) if c.split else c.x.astype(f32)
        acc = np.zeros((c.n_out, H), f32)
        for j in range(c.group):
            acc = acc + v.reshape(c.n_out, c.group, H)[:, j]
        a = acc * (f32(1.0) / f32(c.group))
        hi = round16(a.astype(np.float64), dtype)
        if not c.split:
            assert I.ratio(hi, c.ref.mean, c.ref.tol) <= 1.0, case
            continue
        lo = round16((a - hi.astype(f32)).astype(np.float64), dtype)
        assert ((c.ref.hi_lo <= hi) & (hi <= c.ref.hi_hi)).all() and I.ratio(hi + lo, c.ref.mean, c.ref.tol_sum) <= 1.0, case


# ---------------------------------------------------------------------------- 3. the wrong rules leave ten times the tolerance
@pytest.mark.parametrize("rule", S.RULES["rmsnorm"])
def test_rmsnorm_rules_are_caught(rule):
    figs = []
    for case in I.RMS + [c for c in I.RMS6]:
        c = I.rms(case) if len(case) == 8 else I.rms6(case)
        bad = S.rmsnorm(c.x, c.w, I.RMS_EPS, c.H, rows=c.rows, n_src=c.n_src, form=c.form, ldx=c.ldx, rule=rule)
        figs.append((case, I.ratio(bad.o, c.ref.o, c.ref.tol)))
    caught("rmsnorm", rule, figs)


@pytest.mark.parametrize("rule", S.RULES["rmsnorm16"])
def test_rmsnorm_16_bit_rules_fail_the_bit_check(rule):
    """The GPU test's check is same16(stored, split16(out_f32)).all(); here the stored bytes are a wrong rule's."""
    failed = []
    for dtype in I.DTYPES:
        for case in I.RMS:
            c = I.rms(case)
            if "l" not in c.outs and rule != "saturate_ignored":
                continue
            o = np.nan_to_num(c.ref.o, nan=0.0).astype(f32)
            hi, lo = S.split16(o, dtype, c.sat)
            bhi, blo = S.split16(o, dtype, c.sat, rule=rule)
            bad = not (S.same16(bhi, hi).all() and S.same16(blo, lo).all())
            failed.append((dtype, case, bad))
            if "f" not in c.outs and rule == "lo_dropped":                      # the hi + lo bound of the cases without an f32 output
                r = I.ratio(bhi + blo, np.nan_to_num(c.ref.o), S.tol_hi_lo(c.ref, dtype))
                print(f"SCORE_KERNEL_RULE kernel=rmsnorm16 rule={rule} dtype={dtype} case={case} ratio={r:.4g}")
                assert r > 10.0 and I.ratio(hi + lo, np.nan_to_num(c.ref.o), S.tol_hi_lo(c.ref, dtype)) <= 1.0
    for dtype, case, bad in failed:
        print(f"SCORE_KERNEL_RULE kernel=rmsnorm16 rule={rule} dtype={dtype} case={case} bit_check_fails={bad}")
    assert any(bad for _, _, bad in failed)
    if rule != "lo_dropped":                                                     # about saturation: exactly the fp16 `massive` cases with saturate on
        assert all(bad == (dtype == "f16" and case[6] == "massive" and case[7] == 1) for dtype, case, bad in failed)


def test_tile_bytes_check_fails_on_a_variant():
    c = I.rms6((384, 3, "H", 0))
    o = c.ref.o.astype(f32)
    _, lo = S.split16(o, "f16")
    good = S.tiles_of(lo)
    assert good.shape == ((3 + 255) // 256 * (384 // 128) * 25600,) and good.any()
    assert (S.tiles_of(S.split16(o, "f16", rule="lo_dropped")[1]) != good).any()
    moved = lo.copy()
    moved[[0, 1]] = moved[[1, 0]]
    assert (S.tiles_of(moved) != good).any()                                     # a neighbour's row in the block
    c = I.rms6((384, 257, "2H", 1))
    _, lo = S.split16(c.ref.o.astype(f32), "bf16", poison=c.ref.poison)
    img = S.tiles_of(lo).reshape(2, 3, 25600)
    assert c.ref.poison.sum() == 2 and (lo[c.ref.poison] == 0).all() and img[1].any()          # row 256 lives in the second tile
    unpoisoned = lo.copy()
    unpoisoned[c.ref.poison] = lo[5]
    assert (S.tiles_of(unpoisoned) != S.tiles_of(lo)).any()


def test_sentinel_check_fails_on_a_written_pad():
    before = np.full((7, 24), 0x7B7B, np.uint16)
    own = np.zeros((7, 24), bool)
    own[:5, :16] = True
    after = before.copy()
    after[:5, :16] = 1
    assert I.untouched(before, after, own)
    for r, col in ((2, 16), (5, 0), (6, 23)):                                    # a pad column, the first row past n_rows, the buffer's last element
        worse = after.copy()
        worse[r, col] = 0
        assert not I.untouched(before, worse, own)


@pytest.mark.parametrize("rule", S.RULES["lse_combine"])
def test_lse_combine_rules_are_caught(rule):
    figs = []
    for case in I.LSE:
        c = I.lse(case)
        with np.errstate(**quiet):
            figs.append((case, I.ratio(S.lse_combine(c.m, c.s, c.ll, c.labels, rule=rule)[0], c.ref, c.tol)))
    caught("lse_combine", rule, figs)


@pytest.mark.parametrize("rule", S.RULES["ce_rows"])
def test_ce_rows_rules_are_caught(rule):
    figs = []
    for case in I.CE:
        c = I.ce(case)
        with np.errstate(**quiet):
            figs.append((case, I.ratio(S.ce_rows(np.nan_to_num(c.buf), c.ld, c.V, c.labels, rule=rule)[0], c.ref, c.tol)))
    caught("ce_rows", rule, figs)


@pytest.mark.parametrize("rule", S.RULES["tvg"])
def test_tvg_rules_are_caught(rule):
    figs = []
    for case in I.TVG:
        c = I.tvg(case)
        figs.append((case, I.ratio(S.tvg_criterion(np.nan_to_num(c.buf), c.ld, c.nv, c.labels, c.n_pairs, c.clips, rule=rule)[0], c.ref, c.tol)))
    caught("tvg", rule, figs)


@pytest.mark.parametrize("rule", S.RULES["segment_mean"])
def test_segment_mean_rules_are_caught(rule):
    figs = []
    for case in I.SEG:
        c = I.seg(case)
        figs.append((case, I.ratio(S.segment_mean(c.lp, c.row_start, c.mode, rule=rule)[0], c.ref, c.tol)))
    caught("segment_mean", rule, figs)


@pytest.mark.parametrize("rule", S.RULES["group_mean"])
def test_group_mean_rules_are_caught(rule):
    figs = []
    for dtype in I.DTYPES:
        for case in I.GM:
            c = I.gm(case, dtype)
            bad = S.group_mean(c.x, c.group, dtype, c.split, rule=rule).mean
            if c.split:                                                          # the GPU test's two checks: hi inside its range, hi + lo inside tol_sum
                hi = round16(bad, dtype)
                lo = round16(bad - hi, dtype)
                r = float("inf") if not ((c.ref.hi_lo <= hi) & (hi <= c.ref.hi_hi)).all() else 0.0
                figs.append(((dtype,) + case, max(r, I.ratio(hi + lo, c.ref.mean, c.ref.tol_sum))))
            else:
                figs.append(((dtype,) + case, I.ratio(round16(bad, dtype), c.ref.mean, c.ref.tol)))
    caught("group_mean", rule, figs)


@pytest.mark.parametrize("rule", S.RULES["assemble"])
def test_assemble_byte_check_fails_on_the_rules(rule):
    differs = [(case, bool((S.assemble(I.asm(case).src, I.asm(case).table, I.asm(case).feats, case[0], case[1], rule=rule) != I.asm(case).ref).any())) for case in I.ASM]
    print(f"SCORE_KERNEL_RULE kernel=assemble rule={rule} byte_check_fails={differs}")
    assert any(d for _, d in differs)
    assert all(d for (H, split), d in differs if split or rule == "feature_index_off_by_one")
    assert (bits16(from_bits16(I.asm((8, 0)).ref, "f16"), "f16") == I.asm((8, 0)).ref).all()             # the table's bit patterns survive the test's own conversions
