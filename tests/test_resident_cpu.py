"""tools/mall_model.py: the Infinity-Cache model behind option RESIDENT_BYTES
(DESIGN.md §7 "Resident window").  Two of its figures are pinned: the share of
the headline step's parameter bytes that HBM serves under today's policy and
with a 192 MB resident window.  (The auto rule needs a shard, so a device: it
is checked in tests/test_resident_gpu.py.)"""
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def model():
    spec = importlib.util.spec_from_file_location("mall_model", os.path.join(ROOT, "tools", "mall_model.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_model_uses_the_bench_window_sets(model):
    sets = model.window_sets()
    assert len(sets) == 16
    for push, pull in sets:
        assert not set(push) & set(pull)            # zero push/pull overlap
        assert len(push) + len(pull) == 100         # every free slot is pulled


def test_model_today(model):
    assert model.hbm_share(0) == pytest.approx(0.73, abs=0.01)


def test_model_resident_192mb(model):
    assert model.hbm_share(192 * model.MB) == pytest.approx(0.52, abs=0.01)


def test_model_oversubscribed_window_is_worse(model):
    fits = model.hbm_share(224 * model.MB)
    over = model.hbm_share(256 * model.MB, cache=224 * model.MIB)
    assert fits == pytest.approx(0.44, abs=0.01)
    assert over > fits + 0.05
