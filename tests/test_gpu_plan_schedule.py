"""The engine's and trainer's plans against tests/golden/plan_schedule.json, recorded by tools/record_plan_schedule.py at the commit
before the plan ops became records (ops.py): per row the fusion key, the op lists ([kind, name, hash of the op's descriptor fields,
meta and buffer wiring]), the lane schedules (lanes, waits, events, joins) and the bits of the outputs and of Trainer.grad.  A
change of launch, launch order, lane, event, descriptor field or result bit shows here; a deliberate one re-records the fixture."""
import importlib.util
import json
import os

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
spec = importlib.util.spec_from_file_location("record_plan_schedule", os.path.join(ROOT, "tools", "record_plan_schedule.py"))
REC = importlib.util.module_from_spec(spec)
spec.loader.exec_module(REC)
with open(REC.FIXTURE) as f:
    FIXTURE = json.load(f)
ROWS = ("bf16_forward", "bf16_detect", "bf16_train", "bf16_train_frozen_backbone", "bf16_train_C4_reduced_and_P6",
        "bf16_fp8_backbone_forward", "f32_forward", "f32_train")


@pytest.fixture(scope="module")
def rows(pkg):
    return REC.build_rows(pkg.__name__)


def test_fixture_holds_the_rows_and_no_null_where_none_is_allowed():
    assert sorted(FIXTURE) == sorted(ROWS)
    for name, row in FIXTURE.items():
        assert all(len(p) == 3 and p[2] for p in row["ops"] + row.get("bops", [])), name
        if name in REC.MUST_REPRODUCE:
            assert row["regression"] and row["classification"], name


def same_ops(got, full, want, what):
    assert [p[:2] for p in got] == [p[:2] for p in want], "%s: another op list" % what
    for i, (g, w) in enumerate(zip(got, want)):
        assert g[2] == w[2], "%s: op %d (%s, %s) differs from the recorded one; it is now %s" % (what, i, g[0], g[1], json.dumps(full[i]))


def close(got, want, bf16):
    """Norms of a tensor whose bits the recording commit did not reproduce: tests/test_gpu_train.py's bounds (bf16: norms within
    10 %; f32: 2e-3 of the tensor's scale)."""
    if bf16:
        return all(0.9 * w <= g <= 1.1 * w for g, w in zip(got, want))
    return all(abs(g - w) <= 2e-3 * max(want) for g, w in zip(got, want))


@pytest.mark.parametrize("name", ROWS)
def test_plan_and_schedule_match_the_recording(rows, name):
    (got, full), want = rows[name], FIXTURE[name]
    assert got["key"] == want["key"]
    same_ops(got["ops"], full["ops"], want["ops"], name + " forward")
    assert got["sched"] == want["sched"]
    assert ("bops" in got) == ("bops" in want)
    if "bops" in want:
        same_ops(got["bops"], full["bops"], want["bops"], name + " backward")
        assert got["bsched"] == want["bsched"]
    for k in REC.HASHES:
        assert (k in got) == (k in want), k
        if k not in want:
            continue
        print("%s.%s: %s (recorded %s)" % (name, k, got[k], want[k]))
        if want[k] is not None:
            assert got[k] == want[k], "%s: other bits in %s" % (name, k)
        elif k == "grad":
            for layer, w in want["stats"][k].items():
                assert close(got["stats"][k][layer], w, name.startswith("bf16")), (name, layer, got["stats"][k][layer], w)
        else:
            assert close(got["stats"][k], want["stats"][k], name.startswith("bf16")), (name, k, got["stats"][k], want["stats"][k])
