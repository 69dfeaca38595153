"""CPU side of the input-gradient tests above 1024 points (tests/atk_large_inputs.py): every case that tests/test_gpu_atk_large.py
runs meets atk_oracle.case_conditions from the float64 oracle alone, and the two identities its bitwise tests rest on hold in the
float64 oracle: a cloud's gradient is the gradient of its winner rows alone, and repeated copies of a cloud leave every winner and
the whole gradient in the first copy.  The per-case numbers are printed (-s); DESIGN 7d and 7g record them."""
import warnings

import numpy as np
import pytest
import torch

import atk_large_inputs as LI
import atk_oracle as AO
import pointnet_oracle as PO

warnings.filterwarnings("ignore", message="Converting a tensor with requires_grad")

CONDITION_CASES = [(c, "logits") for c in LI.LARGE_CASES] + [(c, "cross_entropy") for c in LI.CE_CASES] + [("ragged", "logits"), ("add", "logits")]


@pytest.fixture(scope="module")
def sd():
    return PO.make_calibrated_weights(0, False)


@pytest.fixture(scope="module")
def W64(sd):
    return PO.to_torch(sd, torch.float64)


def case_id(p):
    return p if isinstance(p, str) else "%dx%d" % p


@pytest.mark.parametrize("name,loss", CONDITION_CASES, ids=lambda p: case_id(p))
def test_large_cases_meet_the_conditions(sd, name, loss):
    """At most 10 % of a case's clouds wholly out and at least half of its gradient-receiving rows judged, from the oracle alone.
    Measured (clouds wholly out, rows judged, e_32 of the gradient): DESIGN 7d, 7g."""
    cl, tg = LI.inputs(sd, name)
    scale = 1.0 / len(cl) if name == "add" else 1.0
    r32, r64, e, e32, ex = AO.run_case(sd, cl, tg, loss, scale=scale)
    whole, judged, live = AO.case_conditions(r64, e, loss)
    agree = sum(AO.masks_agree(a, b) for a, b in zip(r32, r64))
    top = max(int(max(r["win_feat"].max(), r["win_stn"].max())) for r in r64)
    print("%s %s: e_32(grad) %.3e, e_act c3 %.1e stn3 %.1e, clouds wholly out %d/%d, rows judged %d of %d (%.0f %%), oracles agree on every "
          "mask in %d/%d clouds, highest winner row %d" % (case_id(name), loss, e32, e["c3"], e["stn3"], whole, len(cl), judged, live,
                                                           100.0 * judged / live, agree, len(cl), top))
    assert e32 > 0                                                     # a cloud on which both oracles agree: the bar is defined
    if name != "add":
        assert top >= min(1024, max(len(c) for c in cl) // 2)          # the case does reach the high tiles


@pytest.mark.parametrize("n", [2561, 10000])
def test_a_cloud_is_its_winner_rows(sd, W64, n):
    """U = the sorted union of both max-pools' winners.  The cloud x[U] has the logits, the loss and on its rows the gradient of x;
    every other row of x receives none."""
    cl, tg = LI.inputs(sd, "ragged")
    i = LI.RAGGED_COUNTS.index(n)
    x, t = cl[i], tg[i]
    for loss in ("logits", "cross_entropy"):
        r = AO.run_cloud(W64, x, t, loss)
        U = np.union1d(r["win_feat"], r["win_stn"])
        s = AO.run_cloud(W64, x[U], t, loss)
        big = np.abs(r["grad"]).max()
        print("%d rows, %s: |U| = %d, highest winner row %d, max |grad| %.3e, |sub - full| %.1e of it"
              % (n, loss, len(U), U[-1], big, np.abs(s["grad"] - r["grad"][U]).max() / big))
        assert big > 0 and U[-1] > min(n, 10000) // 2
        assert np.array_equal(np.searchsorted(U, r["win_feat"]), s["win_feat"]) and np.array_equal(np.searchsorted(U, r["win_stn"]), s["win_stn"])
        assert np.abs(s["logits"] - r["logits"]).max() <= 1e-12 * np.abs(r["logits"]).max() and abs(s["loss"] - r["loss"]) <= 1e-12 * abs(r["loss"])
        assert np.abs(s["global_feat"] - r["global_feat"]).max() <= 1e-12 * np.abs(r["global_feat"]).max()
        assert np.abs(s["grad"] - r["grad"][U]).max() <= 1e-12 * big
        assert not np.delete(r["grad"], U, 0).any()


@pytest.mark.parametrize("base,n", [(300, 2500), (257, 10000)])
def test_repeated_copies_leave_everything_in_the_first(sd, W64, base, n):
    """A cloud of `base` rows repeated to n rows: torch.max takes the lowest index among equal values, so every winner lies in the
    first copy, which receives the base cloud's own gradient; the other copies receive none."""
    x, t, tiled = LI.tiled_cloud(sd, base, n)
    a, r = AO.run_cloud(W64, x, t), AO.run_cloud(W64, tiled, t)
    big = np.abs(a["grad"]).max()
    print("%d rows repeated to %d: highest winner row %d, |tiled - base| %.1e of max |grad| %.3e"
          % (base, n, max(r["win_feat"].max(), r["win_stn"].max()), np.abs(r["grad"][:base] - a["grad"]).max() / big, big))
    assert big > 0 and r["win_feat"].max() < base and r["win_stn"].max() < base
    assert np.array_equal(r["win_feat"], a["win_feat"]) and np.array_equal(r["win_stn"], a["win_stn"])
    assert np.abs(r["grad"][:base] - a["grad"]).max() <= 1e-12 * big and not r["grad"][base:].any()
    assert np.abs(r["logits"] - a["logits"]).max() <= 1e-12 * np.abs(a["logits"]).max()

