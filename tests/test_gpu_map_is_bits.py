"""The MAP post-fit entries that share the importance sampler (mdfit_map_laplace,
mdfit_map_psis, mdfit_map_waic, mdfit_map_pred, mdfit_map_evidence and their
_adapt forms) return, on the GPU, the bits of the commit before the sampler's
copies in the four kernels became one core (csrc/mdfit_mapis.h): every record
in full and the SHA-256 of every tap, on 64 taxa of generate(300, seed=21) and
one crafted taxon with y > N, at S = 25 (plain), S = 65 (one draw past the
64-lane stride, two rounds) and S = 256 (plain, and four rounds), seed 0 and
index_base 7.

The fixture tests/golden/map_is_bits_parent.npz was recorded from the parent
commit on a GPU by tools/record_map_is_bits_golden.py, never from the code
under test; the inputs, the configurations and the calls are that tool's.
"""

from __future__ import annotations

import importlib.util

import numpy as np
import pytest

from tests.helpers import GOLDEN

ROOT = GOLDEN.parents[1]
PARENT = "3db158e"


def _tool():
    # the inputs and the calls are defined once, in the tool that recorded the fixture
    path = ROOT / "tools" / "record_map_is_bits_golden.py"
    spec = importlib.util.spec_from_file_location("record_map_is_bits_golden", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


TOOL = _tool()


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN / "map_is_bits_parent.npz")


def test_fixture_names_the_parent_and_covers_every_kind(golden):
    assert (GOLDEN / "map_is_bits_parent.npz").stat().st_size < 1_000_000
    assert str(golden["commit"]).startswith(PARENT)
    idx = golden["indices"]
    assert idx.shape == (TOOL.N_TAXA,) and len(set(idx.tolist())) == TOOL.N_TAXA
    assert idx.min() >= 0 and idx.max() < TOOL.N_POOL
    T = TOOL.N_TAXA + 1
    st = golden["rec/status"]
    assert st.shape == (T,) and st[-1] != 0 and (st[:-1] == 0).sum() > 32
    for kind in TOOL.KINDS:
        assert golden[f"kind/{kind}"].size > 0, kind
    # an invalid null row, a valid proposal refused in round 0: recorded, unless none of the pool's taxa has one
    for kind in TOOL.NOTED:
        assert golden[f"kind/{kind}"].size > 0 or int(golden[f"{kind}_in_pool"]) == 0, kind
    for name, (_S, _R, rounds) in TOOL.CONFIGS.items():
        recs = ["psis", "waic", "evid", "prec", "ppred"]
        recs += ["psis_adapt", "waic_adapt", "evid_adapt", "pred_adapt"] if rounds is not None else []
        for r in recs:
            assert golden[f"rec/{name}/{r}"].shape[0] == T and golden[f"rec/{name}/{r}"].dtype.kind == "i"
        for tap in ("psis_draws", "waic_draws", "evid_draws", "pointwise", "index", "counts"):
            assert len(str(golden[f"sha/{name}/{tap}"])) == 64
    assert golden["rec/lap"].shape == (T, 3, 8) and len(str(golden["sha/gh"])) == 64 and len(str(golden["sha/u"])) == 64
    # the fixture's kinds are what the tool reads off the fixture's own records
    rec = {k[4:]: golden[k] for k in golden.files if k.startswith("rec/")}
    rec = {k: (v.view(np.float64) if v.dtype == np.int64 else v) for k, v in rec.items()}
    kinds = TOOL.kinds(rec)
    for kind in TOOL.REC_KINDS:
        assert np.flatnonzero(kinds[kind]).tolist() == golden[f"kind/{kind}"].tolist(), kind


@pytest.fixture(scope="module")
def computed(golden):
    """Every entry in every configuration on the fixture's taxa, once."""
    import torch

    if not torch.cuda.is_available():
        pytest.fail("gpu test selected but no HIP device is visible")
    from metadamage_amd import _lib, engine, synthetic

    y, N, mm = TOOL.inputs(synthetic, golden["indices"])
    rec, tap = TOOL.run(engine, _lib, torch, y, N, mm)
    for a in (*rec.values(), *tap.values()):
        a.setflags(write=False)
    return rec, tap


def _assert_same(golden, computed, names_rec, names_tap):
    rec, tap = computed
    bad = []
    for name in names_rec:
        got, want = TOOL.bits(rec[name]), golden[f"rec/{name}"]
        assert got.shape == want.shape and got.dtype == want.dtype, name
        n = int((got != want).sum())
        print(f"{name}: {n} of {got.size} words differ from the parent's bits")
        if n:
            bad.append(name)
    for name in names_tap:
        same = TOOL.digest(tap[name]) == str(golden[f"sha/{name}"])
        print(f"{name}: SHA-256 {'equal to' if same else 'differs from'} the parent's")
        if not same:
            bad.append(name)
    assert not bad, bad


@pytest.mark.gpu
def test_fit_and_laplace_return_the_parent_commits_bits(golden, computed):
    _assert_same(golden, computed, ["status", "lap"], ["gh", "u"])
    # the rows the fixture names as invalid by their proposal / refused in round 0 are those rows here
    rec, tap = computed
    kinds = TOOL.tap_kinds(rec["status"], tap)
    for kind in TOOL.TAP_KINDS:
        assert np.flatnonzero(kinds[kind]).tolist() == golden[f"kind/{kind}"].tolist(), kind


@pytest.mark.gpu
@pytest.mark.parametrize("config", sorted(TOOL.CONFIGS))
def test_entries_return_the_parent_commits_bits(golden, computed, config):
    rec, tap = computed
    names_rec = sorted(k for k in rec if k.startswith(config + "/"))
    names_tap = sorted(k for k in tap if k.startswith(config + "/"))
    assert len(names_rec) == (9 if TOOL.CONFIGS[config][2] is not None else 5) and len(names_tap) == 6
    assert {f"rec/{k}" for k in names_rec} == {k for k in golden.files if k.startswith(f"rec/{config}/")}
    assert {f"sha/{k}" for k in names_tap} == {k for k in golden.files if k.startswith(f"sha/{config}/")}
    _assert_same(golden, computed, names_rec, names_tap)
