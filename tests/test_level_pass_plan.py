"""The launch plan of the level grower's passes (rgbm_level_pass_plan: pure arithmetic, no device) for the two bench shapes, for the distinct-row view
of the flagship (2 495 053 rows with multiplicities) and for a 10 000-row table, every target of each:

  * every gx (row blocks per class tree; root pass and level passes) is a multiple of 8, and no workgroup gets more than 2^22 rows;
  * part_items covers the partials of the root pass and of every level-pass launch;
  * the launches of a level share one gx;
  * RGBM_LV_BLOCKS / RGBM_MT_BLOCKS override the choice (rounded up to a multiple of 8);
  * the grid rule knows what a workgroup costs: no launch both exceeds one round of 256 workgroups and gives a workgroup less modelled row-loop time
    than its modelled fixed time.  The rule cannot go below its lower bound (8 row blocks, or what 2^22 rows per workgroup ask for): where G class
    tree groups x that bound already exceed a round -- the K = 64 target of a 10 000-row table at levels 5 and 6 -- the launch has to sit AT the bound.
"""
import os

import numpy as np
import pytest

from tests.synth import make_table

SHAPES = [("10m16", 16, 42, 10_000_000, False), ("100m32 rank shard", 32, 43, 12_500_000, False), ("100m32", 32, 43, 100_000_000, False),
          ("10m16 distinct-row view", 16, 42, 2_495_053, True), ("10 000 rows", 16, 42, 10_000, False)]
SWITCHES = ["RGBM_LV_BLOCKS", "RGBM_MT_BLOCKS", "RGBM_MT_TREES", "RGBM_LV_LDS", "RGBM_MT_ROT", "RGBM_MT_REP", "RGBM_MT_ACC2", "RGBM_MT_ROT_COPIES2", "RGBM_MT_ROT_TMIN"]


def _plans(cols, seed, rows, with_mult):
    from repair import _native as N
    _, _, cards = make_table(64, cols, seed=seed)
    for t in range(cols):
        K = int(cards[t])
        nbins = [int(cards[c]) + 1 for c in range(cols) if c != t]          # (every column has NULLs: one NaN bin each)
        yield t, (1 if K == 2 else K), N.level_pass_plan(nbins, rows, 1 if K == 2 else K, 7, with_mult)


@pytest.fixture(autouse=True)
def _no_switches(monkeypatch):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)


@pytest.mark.parametrize("name,cols,seed,rows,with_mult", SHAPES, ids=[s[0] for s in SHAPES])
def test_plan_invariants(name, cols, seed, rows, with_mult):
    gx_lo = max(8, (-(-rows // (1 << 22)) + 7) // 8 * 8)
    for t, K, p in _plans(cols, seed, rows, with_mult):
        assert p["root_gx"] % 8 == 0 and p["root_gx"] >= gx_lo and rows / p["root_gx"] <= (1 << 22), (t, p["root_gx"])
        assert p["part_items"] >= K * p["root_gx"]
        assert sorted(set(L["level"] for L in p["launches"])) == list(range(1, 7))
        for level in range(1, 7):
            ls = [L for L in p["launches"] if L["level"] == level]
            assert len(set(L["gx"] for L in ls)) == 1, (t, level, ls)
            assert sum(L["route"] for L in ls) == 1 and ls[0]["route"] == 1
            for L in ls:
                assert L["gx"] % 8 == 0 and L["gx"] >= gx_lo and rows / L["gx"] <= (1 << 22), (t, L)
                assert p["part_items"] >= K * L["gx"] * (1 << (level - 1)), (t, L)
                assert L["G"] * L["T"] >= K and (L["G"] - 1) * L["T"] < K
                over_a_round = L["G"] * L["gx"] > 256
                assert not (over_a_round and L["t_rows_us"] < L["t_fix_us"] and L["gx"] > gx_lo), (name, t, L)
        assert not (p["root_workgroups"] > 256 and p["root_t_rows_us"] < p["root_t_fix_us"] and p["root_gx"] > gx_lo), (name, t, p["root_gx"])


@pytest.mark.parametrize("blocks,want", [(8, 8), (20, 24), (24, 24), (152, 152)])
def test_block_switches_override_the_choice(blocks, want, monkeypatch):
    monkeypatch.setenv("RGBM_MT_BLOCKS", str(blocks))
    for t, K, p in _plans(16, 42, 2_495_053, True):
        assert all(L["gx"] == want for L in p["launches"]) and p["part_items"] >= K * want * 32
    monkeypatch.delenv("RGBM_MT_BLOCKS")
    monkeypatch.setenv("RGBM_LV_BLOCKS", str(blocks))
    for t, K, p in _plans(16, 42, 2_495_053, True):
        assert p["root_gx"] == want and p["part_items"] >= K * want
