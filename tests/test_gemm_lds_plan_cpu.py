"""Routing of the LDS-tiled GEMM engine, pinned without a GPU: rlrep_gemm_plan (which launches nothing) over a grid of products -- the three layout
pairs the engine accepts and one it refuses, every layer of the five agents at the BASELINE.json dimensions, leading dimensions that set each scalar
side, both sides of every routing threshold -- must answer (engine, tile, splits, kchunk, scalar_sides) EXACTLY as the library of the commit
before the tile-kind table did, under the default switches and under each RLREP_DISABLE token the routing reads.  The expected answers are
tests/golden/gemm_lds_plan.json, written by tests/golden/make_gemm_lds_plan.py from that earlier library."""
import json

import pytest

from fixture_io import GOLD      # puts tests/golden on sys.path
import make_gemm_lds_plan as mk


@pytest.fixture(scope='module')
def fixture():
    with open(mk.FIXTURE) as f:
        return json.load(f)


def _row(layout, R, Cn, K):
    return [layout[0], layout[1], R, Cn, K, *mk._ld(layout, R, Cn, K)]


def test_fixture_covers_the_grid_and_every_tile_kind(fixture):
    """Conditions on the FIXTURE, so that a thin grid cannot pass by accident."""
    assert mk.FIXTURE.startswith(GOLD)
    assert fixture['grid'] == mk.grid()
    assert sorted(fixture['plans']) == sorted(mk.SETTINGS)
    for s in mk.SETTINGS:
        assert len(fixture['plans'][s]) == len(fixture['grid']), s
    pairs = lambda s: {(p[0], p[1]) for p in fixture['plans'][s]}
    assert pairs('') == {(0, 16), (1, 128), (2, 32), (2, 64), (2, 128), (2, 256)}
    assert (1, 64) in pairs('x3s') and (1, 64) in pairs('x3')
    assert pairs('gemm_lds') == {(0, 16)}
    layouts = {(r[0], r[1]) for r in fixture['grid']}
    assert layouts == {mk.FWD, mk.DX, mk.DW, mk.REFUSED}
    assert all(p[0] == 0 for r, p in zip(fixture['grid'], fixture['plans']['']) if (r[0], r[1]) == mk.REFUSED)
    sides = {p[4] for p in fixture['plans']['']}
    assert {0, 1, 2, 4} <= sides, sides                       # every scalar side alone, and none
    assert any(p[2] > 1 for p in fixture['plans'][''])


@pytest.mark.parametrize('layout,R,Cn,K,engine,tile', [
    (mk.FWD, 4096, 4096, 4096, 2, 256),
    (mk.FWD, 2560, 3840, 1024, 2, 128),
    (mk.FWD, 2048, 2048, 128, 1, 128),
    (mk.FWD, 256, 256, 4096, 2, 64),
    (mk.FWD, 256, 1024, 1024, 2, 32),
    (mk.FWD, 64, 64, 64, 0, 16), (mk.DX, 64, 64, 64, 0, 16), (mk.DW, 64, 64, 64, 0, 16),
])
def test_routes_worked_out_by_hand(fixture, layout, R, Cn, K, engine, tile):
    """The default-switch routes derived by reading rl_gemm_lds_route are what the earlier library answered (and so what the test below demands)."""
    p = fixture['plans'][''][fixture['grid'].index(_row(layout, R, Cn, K))]
    assert (p[0], p[1]) == (engine, tile), p
    if (R, Cn, K) == (256, 256, 4096):
        assert p[2] > 1, p                                    # split along K
    if tile == 32:
        assert (p[2], p[3]) == (1, K), p                      # the 32 x 32 tile carries no slabs


@pytest.mark.parametrize('setting', mk.SETTINGS)
def test_plan_equals_the_earlier_library(fixture, setting, monkeypatch):
    from rlrep_amd import _lib
    monkeypatch.delenv('RLREP_ENABLE', raising=False)
    monkeypatch.setenv('RLREP_DISABLE', setting)
    wrong = []
    for row, want in zip(fixture['grid'], fixture['plans'][setting]):
        got = mk.plan(_lib.lib, row)
        if got != want:
            wrong.append((row, got, want))
    assert not wrong, (setting, len(wrong), wrong[:5])
