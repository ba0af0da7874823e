"""tests/attention_profiles.py without a GPU: every (profile, geometry, position) combination that
tests/test_gpu_attention_scores.py launches satisfies the precondition its profile states on the float64 reference, and
the reference's tolerance discriminates: four deliberately wrong fp32 softmaxes over split partials (m, l, o), kept
as the kernels keep them, are each rejected by the profile that exists to catch them and accepted by the N(0, 1) inputs
every earlier attention test draws, where that is the point being made."""

import math

import numpy as np
import pytest

import attention_profiles as ap

_GEOM_IDS = lambda g: f"H{g[0]}-G{g[1]}-hs{g[2]}-x{g[3]}"  # noqa: E731
_CASES = [(form, g) for form in ap.FORMS for g in ap.geoms(form)]
_IDS = [f"{form}-{_GEOM_IDS(g)}" for form, g in _CASES]


def _check(form, H, G, hs, spec):
    c = ap.build(form, H, G, hs, spec)
    r = ap.reference(c.q, c.k, c.v, [c.p], c.scale)
    ap.check_case(c, r)
    assert np.all(np.isfinite(r.ref)) and np.all(r.tol > 0)
    if c.profile == "one_hot":  # the reference itself is V[g, j_h]
        for h in range(H):
            assert np.all(np.abs(r.ref[0, h] - c.v[h // (H // G), c.hot[h]]) <= 0.1 * r.tol[0, h]), (h, c.hot[h])
    return c, r


@pytest.mark.parametrize("form,geom", _CASES, ids=_IDS)
def test_sweep_and_profile_cases_meet_their_preconditions(form, geom):
    H, G, hs, _ = geom
    seen = set()
    for spec in ap.sweep_specs(H, G):
        _check(form, H, G, hs, spec)
        seen.update(spec["hot"])
    assert seen == set(range(ap.SWEEP_P + 1)), "every key is the hot key of some head"
    for p in ap.PROFILE_P:
        for spec in ap.profile_specs(H, G, p):
            _check(form, H, G, hs, spec)
    if form == "kv8":
        for spec in ap.spread_specs(H, G):
            c, _ = _check(form, H, G, hs, spec)
            for s in (c.k_scale, c.v_scale):
                assert s.max() / s.min() >= 2.0 ** 13


@pytest.mark.parametrize("form,geom", _CASES, ids=_IDS)
def test_long_cache_cases_meet_their_preconditions(form, geom):
    H, G, hs, _ = geom
    names = set()
    for p, n_splits in ap.long_runs():
        for spec in ap.long_specs(H, G, p, n_splits, form != "rows"):
            _check(form, H, G, hs, spec)
            names.add(spec.get("name"))
    want = {"one-row-group", "one-wave", "two-waves", "two-splits", "two-rounds"}
    if form != "rows":
        want |= {"new-key-and-neighbour", "new-key-and-key-0"}
    assert want <= names


def test_long_hot_keys_sit_on_the_split_edges():
    for p, n_splits in ap.long_runs():
        chunk = -(-(p + 1) // n_splits)
        hot = ap.long_hot(8, 1, p, n_splits)
        assert {0, chunk - 1, chunk, p - 1, p} <= set(hot)
    # 2048 and 2304 keys fill all 256 splits of 8 and 9 keys: the extra run is the one with splits that hold no key
    assert not any(lo == hi for p in ap.LONG_P for lo, hi in ap.split_ranges(p, 256))
    assert sum(lo == hi for lo, hi in ap.split_ranges(*ap.LONG_EXTRA[0])) == 28


@pytest.mark.parametrize("hs", ap.PREFILL_HS)
@pytest.mark.parametrize("H,G", ap.PREFILL_GEOMS)
@pytest.mark.parametrize("T,start", ap.PREFILL_ROWS)
def test_prefill_cases_meet_their_preconditions(T, start, H, G, hs):
    for kind in ap.PREFILL_KINDS:
        for pair in (ap.prefill_pairs(T, start) if kind == "two_peaks" else [None]):
            c = ap.prefill_case(kind, T, start, H, G, hs, T, start, H, G, hs, pair=pair)
            r = ap.reference(c.q, c.k, c.v, c.positions, c.scale, mfma=True)
            assert c.checks or kind in ("ramp_up", "sink", "mixed") and start + T <= 127
            for fn, t, h, extra in c.checks:
                fn(r, t, h, *extra)
            if kind in ("ramp_up", "sink", "mixed"):  # every row, however short: its extreme key is where it belongs
                for t in range(T):
                    s = r.scores[t, :, :start + t + 1]
                    up = kind == "ramp_up" or (kind == "mixed" and t % 2 == 1)
                    assert np.all(s.argmax(axis=-1) == (start + t if up else 0))
    hot = ap.prefill_hot(T, start)
    last = start + T - 1
    assert hot[-1] == last and hot[-2] == last - 2 and hot[-8] == 0
    assert all(0 <= j <= start + t for t, j in enumerate(hot))


# ------------------------------------------------------------------------------------------------ mutation checks
H_, G_, HS_ = 8, 2, 128
SCALE_ = 1.0 / math.sqrt(HS_)


def _verdict(c, n_splits, mutation):
    """(finite, within tolerance) of the fp32 split softmax under ``mutation`` against the float64 reference."""
    r = ap.reference(c.q, c.k, c.v, [c.p], c.scale)
    y = ap.split_softmax(c.q[0], c.k, c.v, c.p, c.scale, n_splits, mutation)
    finite = bool(np.all(np.isfinite(y)))
    return finite, finite and bool(np.all(np.abs(y - r.ref[0]) <= r.tol[0]))


def _normal_case(p):
    """What every earlier test draws: q, k, v ~ N(0, 1)."""
    return ap.Case(profile="normal", q=ap.normal((1, H_, HS_), 901), k=ap.normal((G_, p + 1, HS_), 902),
                   v=ap.normal((G_, p + 1, HS_), 903), p=p, scale=SCALE_)


def _case(profile, p=ap.SWEEP_P, **kw):
    spec = dict(profile=profile, p=p, hot=ap.default_hot(H_, p), pairs=ap.default_pairs(H_, G_, p))
    spec.update(kw)
    return ap.build("rows", H_, G_, HS_, spec)


@pytest.mark.parametrize("n_splits", [1, 7, 36])
def test_the_correct_split_softmax_passes_every_profile(n_splits):
    assert _verdict(_normal_case(ap.SWEEP_P), n_splits, None) == (True, True)
    for profile in ap.PROFILES:
        assert _verdict(_case(profile), n_splits, None) == (True, True), profile
    for spec in ap.sweep_specs(H_, G_):
        assert _verdict(ap.build("rows", H_, G_, HS_, spec), n_splits, None) == (True, True)


def test_mutation_no_max_subtraction():
    """Invisible on N(0, 1) inputs; non-finite on both offsets (2^160 overflows fp32, 2^-160 flushes every weight)."""
    for n_splits in (1, 7):
        assert _verdict(_normal_case(ap.SWEEP_P), n_splits, "no_max") == (True, True)
        assert _verdict(_case("offset_pos"), n_splits, "no_max")[0] is False
        assert _verdict(_case("offset_neg"), n_splits, "no_max")[0] is False


def test_mutation_merge_keeps_the_larger_maximum():
    """A hot key alone hides it; two peaks or a runner-up in different partials do not."""
    n_splits, p = 7, ap.SWEEP_P
    chunk = -(-(p + 1) // n_splits)
    apart = [(5 + h % 4, 3 * chunk + 5 + h % 4) for h in range(H_)]  # splits 0 and 3
    assert _verdict(_case("one_hot"), n_splits, "keep_larger") == (True, True)
    assert _verdict(_case("two_peaks", pairs=apart), n_splits, "keep_larger") == (True, False)
    assert _verdict(_case("runner_up", pairs=apart), n_splits, "keep_larger") == (True, False)
    assert _verdict(_case("two_peaks", pairs=apart), n_splits, None) == (True, True)


def test_mutation_merge_forgets_to_rescale_l():
    for n_splits in (7, 36):
        assert _verdict(_case("ramp_up"), n_splits, "stale_l") == (True, False)
        assert _verdict(_case("sink"), n_splits, "stale_l") == (True, False)


def test_mutation_split_range_drops_its_last_key():
    """Some launch of the every-key sweep puts a hot key on the last key of a split: rejected there, and only there."""
    n_splits = 7
    ends = {hi - 1 for lo, hi in ap.split_ranges(ap.SWEEP_P, n_splits)}
    rejected = 0
    for spec in ap.sweep_specs(H_, G_):
        ok = _verdict(ap.build("rows", H_, G_, HS_, spec), n_splits, "drop_last")[1]
        assert ok == (not ends & set(spec["hot"])), spec["hot"]
        rejected += not ok
    assert rejected >= len(ends) // H_ and rejected > 0
