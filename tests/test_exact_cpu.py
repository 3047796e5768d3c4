"""The conditions under which tests/test_exact_gpu.py may demand exact results, checked against the references alone (no GPU),
and the helpers of tests/exact_inputs.py against planted errors."""
import pytest
import torch

from tests import exact_inputs as X


@pytest.mark.parametrize("name", sorted(X.LINEAR_CASES))
def test_linear_cases_stay_exact(name):
    c = X.LINEAR_CASES[name]
    acc, epi = X.lin_bounds(c)
    assert acc < X.F32_EXACT and epi < X.F32_EXACT, "a partial sum could leave the exact range of fp32"
    assert c["alpha"] in (1.0, 0.5, 2.0) and (c["alpha"] != 0.5 or c["wmul"] % 2 == 0), "alpha * sum must stay an integer"
    if not c["out_f32"]:
        assert epi <= X.F16_EXACT, f"|ref| may reach {epi}: not every integer is an fp16 there"
    p = X.lin_problem(c, M=min(c["M"], 300) if c["M"] else 300)          # the bounds hold for every M; the reference of a few rows shows them
    assert int(p["ref"].abs().max()) <= epi
    assert float(p["x"].abs().max()) <= c["ax"] and float(p["w"].abs().max()) <= c["aw"] * c["wmul"]
    assert int(p["ref"].abs().max()) > 8, "a degenerate reference would prove nothing"


@pytest.mark.parametrize("name", sorted(X.UNITS_CASES))
def test_units_cases_stay_exact(name):
    units, unit_rows, N, K = X.UNITS_CASES[name]
    x, w, b, ref, bound = X.units_problem(units, min(unit_rows, 64), N, K)
    assert bound <= X.F16_EXACT and int(ref.abs().max()) <= bound
    assert all(not torch.equal(w[u], w[u + 1]) for u in range(units - 1)), "every unit needs its own weights"
    # a tile that reads the next unit's weights is an exact mismatch: the rows of unit 0 under the weights of unit 1 differ
    wrong = (x[:min(unit_rows, 64)].double() @ w[1].double().t() + b[1].double()).to(torch.int64)
    assert not torch.equal(wrong, ref[:min(unit_rows, 64)])


@pytest.mark.parametrize("name", sorted(X.CONV_CASES))
def test_conv_cases_stay_exact(name):
    c = X.CONV_CASES[name]
    acc, epi = X.conv_bounds(c)
    assert acc < X.F32_EXACT and epi <= X.F16_EXACT
    p = X.conv_problem(c)
    assert int(p["ref"].abs().max()) <= epi and int(p["ref"].abs().max()) > 8
    assert all(k % 64 == 0 for k in c["tails"])


@pytest.mark.parametrize("nk,nq,groups,heads", [(77, 100, 2, 2), (135, 64, 1, 1), (4096, 128, 1, 1), (4160, 128, 1, 1), (64, 64, 2, 3), (25, 25, 3, 2)])
def test_one_hot_inputs_have_the_logit_gap(nk, nq, groups, heads):
    q, k, v, perm = X.one_hot_problem(groups, heads, nk, nq, seed=nk)
    assert float(q.abs().max()) == X.ONE_HOT_BETA and float(k.abs().max()) == 1.0
    assert X.one_hot_gap(q, k, perm, 0.125) >= X.ONE_HOT_GAP_NATS
    # the losing keys together hold less than 1e-9 of the probability (the fp32 row sum stays 1), and each of them is below half
    # the smallest fp16 subnormal: packed to fp16 for the matrix pipe it is exactly 0, so a code of 0 comes out as exactly 0
    lose = float(torch.exp(torch.tensor(-X.ONE_HOT_GAP_NATS, dtype=torch.float64)))
    assert nk * lose < 1e-9 and lose < 2.0 ** -25
    # V codes: neighbours in key and in column differ by at least 1, heads and groups differ
    c = X.v_codes(200).double()
    assert float((c[1:] - c[:-1]).abs().min()) >= 1 and float((c[:, 1:] - c[:, :-1]).abs().min()) >= 1 and float(c.abs().max()) <= 30
    for gi in range(groups):
        for h in range(heads):
            for g2, h2 in ((gi, (h + 1) % heads), ((gi + 1) % groups, h)):
                if (g2, h2) != (gi, h):
                    assert float((v[gi, :, h].double() - v[g2, :, h2].double()).abs().min()) >= 1
    if nk >= 128:
        tiles = perm[0, 0] // 64
        assert int((tiles[1:] != tiles[:-1]).sum()) >= nq // 4, "the selected keys must jump between key tiles"


def test_uniform_inputs():
    for nk in X.FLASH_UNIFORM_NK + X.TEMPORAL_UNIFORM_T:
        v, mean = X.uniform_values(nk, 64)
        assert nk * 30 < X.F32_EXACT and torch.equal(v.double().sum(0) / nk, mean)
        # one padding key of value PAD_FINITE counted by mistake moves the mean by far more than an fp16 ulp
        off = ((v.double().sum(0) + X.PAD_FINITE) / (nk + 1) - mean).abs()
        assert bool((off > 4 * X.f16_ulp(mean)).all())
    u = X.f16_ulp(torch.tensor([1.0, 1.5, 2.0, 1000.0, 0.0, 3e-6], dtype=torch.float64))
    assert u.tolist() == [2.0 ** -10, 2.0 ** -10, 2.0 ** -9, 0.5, 2.0 ** -24, 2.0 ** -24]


def test_int_tensor_is_reproducible_and_in_range():
    a, b = X.int_tensor((50, 40), -3, 3, 5), X.int_tensor((50, 40), -3, 3, 5)
    assert torch.equal(a, b) and a.dtype == torch.float16 and float(a.min()) == -3 and float(a.max()) == 3
    assert torch.equal(a, a.round()) and not torch.equal(a, X.int_tensor((50, 40), -3, 3, 6))


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32])
def test_assert_exact_fails_on_one_planted_element(dtype):
    ref = X.lin_problem(X.LINEAR_CASES["cfg0"])["ref"]
    out = ref.to(dtype)
    X.assert_exact(out, ref, "clean")
    out[130, 129] += 1                      # row 2 of the second row tile, column 1 of the second column tile
    with pytest.raises(AssertionError) as e:
        X.assert_exact(out, ref, "planted")
    msg = str(e.value)
    assert "1 of" in msg and "(130, 129)" in msg and "mod 128: row 2 col 1" in msg and "mod 64: row 2 col 1" in msg and "mod 256: row 130 col 129" in msg
    out[130, 129] = float("nan")
    with pytest.raises(AssertionError):
        X.assert_exact(out, ref, "planted NaN")
    with pytest.raises(AssertionError):     # a reference that fp16 cannot hold is a mistake of the test, not a pass
        X.assert_exact(torch.full((2, 2), 2049.0, dtype=torch.float16), torch.full((2, 2), 2049, dtype=torch.int64), "unrepresentable")


def test_assert_elementwise_fails_on_one_planted_element():
    ref = torch.linspace(-4, 4, 64 * 300, dtype=torch.float64).view(300, 64)
    bound = X.f16_ulp(ref)
    out = ref.half()
    X.assert_elementwise(out, ref, bound, "clean")
    bad = out.clone()
    bad[257, 3] += 4 * float(bound[257, 3])
    with pytest.raises(AssertionError) as e:
        X.assert_elementwise(bad, ref, bound, "planted")
    assert "1 of" in str(e.value) and "(257, 3)" in str(e.value) and "mod 256: row 1 col 3" in str(e.value)
    bad = out.clone()
    bad[0, 0] = float("nan")
    with pytest.raises(AssertionError):
        X.assert_elementwise(bad, ref, bound, "planted NaN")
    # a whole-tensor norm would not have seen the planted element
    e2 = float((out.double() - ref).norm() / ref.norm())
    bad = out.clone()
    bad[257, 3] += 4 * float(bound[257, 3])
    assert float((bad.double() - ref).norm() / ref.norm()) <= max(2e-3, 2 * e2)
