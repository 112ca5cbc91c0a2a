"""The order in which a member-axis call of an ensemble looks at its arguments: every case hands one call TWO defects at once and asserts
the code of the one that is checked first. Each call orders its checks differently (include/wxsim.h says what is refused, the entry
points in csrc/wx_ens_*.h in which order), and a host that branches on the code sees that order. Codes: -1 invalid, -4 range, -5 state.
The ensemble is the one of test_refusals of tests/test_ensemble_statistics_gpu.py: 57 x 9 cells, three members, member 2 never uploaded."""
import numpy as np
import pytest

from test_ensemble_statistics_gpu import make_ensemble, member_specs

pytestmark = pytest.mark.gpu

X, Y = 57, 9
OUTSIDE = (1, 0, X, 1)  # one column past the right edge
GOOD, BAD_FIELD = "BASE_CUR", "WALL_CUR"


@pytest.fixture(scope="module")
def ens(pkg):
    e = make_ensemble(pkg, member_specs(pkg, X, Y, 3)[:2] + [None])  # member 2 is never uploaded
    yield e
    e.close()


def refused(pkg, code, call, *a, **kw):
    with pytest.raises(pkg.engine.WxError) as ei:
        call(*a, **kw)
    assert ei.value.code == code, (a, kw, str(ei.value))
    return str(ei.value)


@pytest.mark.parametrize("name", ["statistics", "save_prior"])
def test_statistics_and_save_prior(pkg, ens, name):
    """field, then rect, then empty selection, then uploaded"""
    if name == "statistics":
        call = lambda field, rect, members: ens.statistics(field, *rect, members=members)  # noqa: E731
    else:
        call = lambda field, rect, members: ens.save_prior(field, rect, members)  # noqa: E731
    refused(pkg, -1, call, BAD_FIELD, OUTSIDE, [0, 1])
    refused(pkg, -4, call, GOOD, OUTSIDE, [0, 2])
    refused(pkg, -4, call, GOOD, OUTSIDE, [])


def test_quantiles(pkg, ens):
    """field, then the descriptor, then rect, then uploaded"""
    msg = refused(pkg, -1, ens.quantiles, BAD_FIELD, [1.5], members=[0, 1])
    assert "WX_FIELD_BASE_CUR" in msg and "WX_FIELD_WATER_CUR" in msg
    msg = refused(pkg, -1, ens.quantiles, GOOD, [1.5], *OUTSIDE, members=[0, 1])
    assert "[0, 1]" in msg
    refused(pkg, -4, ens.quantiles, GOOD, [0.5], *OUTSIDE, members=[0, 2])


def test_scores(pkg, ens):
    """field, then the selection, then truth-is-member, then truth's shape, then rect, then uploaded"""
    refused(pkg, -1, ens.scores, GOOD, ens[0], *OUTSIDE, members=[0, 1])
    refused(pkg, -4, ens.scores, GOOD, ens[1], *OUTSIDE, members=[0, 2])


def test_assimilate(pkg, ens):
    """the descriptor, then fewer than two, then uploaded"""
    msg = refused(pkg, -1, ens.assimilate, [(GOOD, 20, 4, 3, 300.0, 0.25)], members=[2])
    assert "takes two" in msg


def test_inflate(pkg, ens):
    """the descriptor, then fewer than two, then rect, then uploaded, then the snapshot"""
    ens.drop_prior(GOOD)
    refused(pkg, -1, ens.inflate, GOOD, 1.5, rect=OUTSIDE, members=[0])
    refused(pkg, -4, ens.inflate, GOOD, 1.5, rect=OUTSIDE, members=[0, 2])
    msg = refused(pkg, -5, ens.inflate, GOOD, 0.5, mode="rtps", members=[0, 2])
    assert "member 2" in msg and "no snapshot" not in msg


def test_covariance(pkg, ens):
    """the descriptor, then fewer than two, then the values, then rect, then uploaded, then the snapshot"""
    ens.drop_prior(GOOD)
    point = [(GOOD, 3, 3, 3)]
    refused(pkg, -1, ens.covariance, GOOD, point, source="prior", rect=OUTSIDE, members=[0])
    refused(pkg, -4, ens.covariance, GOOD, point, source="prior", rect=OUTSIDE, members=[0, 2])
    msg = refused(pkg, -5, ens.covariance, GOOD, point, source="prior", members=[0, 2])
    assert "member 2" in msg and "no snapshot" not in msg
    msg = refused(pkg, -1, ens.covariance, GOOD, [np.array([1.0, np.nan, 0.0])], rect=OUTSIDE, members=[0, 1])
    assert "values predictor" in msg


def test_perturb(pkg, ens):
    """the descriptor (which holds the rectangle), then the empty selection"""
    refused(pkg, -4, ens.perturb, GOOD, 0.1, rect=OUTSIDE, members=[])
    assert "scale" in refused(pkg, -1, ens.perturb, GOOD, 0.1, scale=0, members=[])


def test_the_ensemble_is_untouched(pkg, ens):
    """no refusal above left anything behind: the uploaded members are served"""
    got = ens.statistics(GOOD, members=[0, 1], want=("count", "n_wall"))
    assert got["count"].shape == (Y, X, 4) and int(got["n_wall"].max()) <= 2
