"""CPU tests of the training state (lft_amd/train.py: check_state / TrainStep.load_state_dict, lft_amd/trainer.py: the state file,
tools/train_dp.py: --resume): every refusal names its field, the save is atomic, the EMA warm-up schedule follows its formula.

A TrainStep cannot be constructed without a GPU (its guard block is written by a kernel), so the receiving side is either the
description check_state takes, or a TrainStep whose fields are set by hand on CPU tensors: an UNGUARDED step loads a state without a
single device call, and every refusal comes before the first one."""
import importlib.util
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from lft_amd import train as T
from lft_amd import trainer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 10
SEGS = [(0, 3, True), (3, 1, False), (4, 6, True)]


def stub_step(guard=False, ema=True):
    """A TrainStep with hand-set fields on the CPU (no constructor: that needs the device)."""
    ts = object.__new__(T.TrainStep)
    ts.net = SimpleNamespace(channels=64, _packed=None)
    ts.lr, ts.betas, ts.eps, ts.weight_decay = 2e-4, (0.9, 0.999), 1e-8, 0.0
    ts.max_grad_norm, ts.guard, ts.math = (1.0 if guard else None), guard, "fp32"
    ts.ema_decay, ts.ema_warmup = (0.999 if ema else None), True
    ts.A, ts.s = 2, 2
    ts.flat_params = torch.arange(N, dtype=torch.float32)
    ts.m, ts.v = torch.zeros(N), torch.zeros(N)
    ts.ema = torch.zeros(N) if ema else None
    ts._segments = list(SEGS)
    ts._guard = None
    ts._counter0 = {"steps_skipped": 0, "steps_clipped": 0}
    ts.t = 0
    return ts


def good_state(guard=False, ema=True):
    sd = {"version": T.STATE_VERSION, "lr": 2e-4, "betas": (0.9, 0.999), "eps": 1e-8, "weight_decay": 0.0,
          "max_grad_norm": 1.0 if guard else None, "guard": guard, "math": "fp32", "ema_decay": 0.999 if ema else None, "ema_warmup": True,
          "A": 2, "scale": 2, "channels": 64, "floats": N, "trainable": [t for _, _, t in SEGS],
          "m": torch.full((N,), 1.0), "v": torch.full((N,), 2.0), "ema": torch.full((N,), 3.0) if ema else None, "t": 7}
    if guard:
        sd.update(steps_applied=5, steps_skipped=2, steps_clipped=1)
    return sd


def own_of(ts):
    own = ts._describe()
    own["ema"] = ts.ema is not None
    return own


def test_a_matching_state_loads_in_place_without_the_device():
    ts = stub_step()
    ptrs = [t.data_ptr() for t in (ts.m, ts.v, ts.ema)]
    sd = good_state()
    assert T.check_state(sd, own_of(ts)) == []
    ts.load_state_dict(sd)
    assert [t.data_ptr() for t in (ts.m, ts.v, ts.ema)] == ptrs, "the buffers were replaced, not written"
    assert ts.t == 7 and torch.equal(ts.m, sd["m"]) and torch.equal(ts.v, sd["v"]) and torch.equal(ts.ema, sd["ema"])
    # what state_dict() of that step holds goes through the same check
    back = ts.state_dict()
    assert set(back) == set(sd) and back["t"] == 7 and back["trainable"] == [True, False, True] and back["floats"] == N
    assert T.check_state(back, own_of(ts)) == []


def change(key, value):
    def f(sd):
        sd[key] = value
    return f


def drop(key):
    def f(sd):
        del sd[key]
    return f


REFUSALS = [  # (what, guarded receiver, receiver keeps an ema, edit of a good state, field the error must name)
    ("another float count", False, True, change("floats", N + 1), "floats"),
    ("another scale", False, True, change("scale", 4), "scale"),
    ("another channel width", False, True, change("channels", 32), "channels"),
    ("another set of frozen tensors", False, True, change("trainable", [True, True, True]), "trainable"),
    ("a newer format", False, True, change("version", T.STATE_VERSION + 1), "version"),
    ("no format version", False, True, drop("version"), "version"),
    ("ema in the state only", False, False, change("ema", torch.zeros(N)), "ema"),
    ("ema in the step only", False, True, change("ema", None), "ema"),
    ("unguarded state into a guarded step", True, True, change("guard", False), "guard"),
    ("guarded state into an unguarded step", False, True, change("guard", True), "guard"),
    ("a guarded state without its counter", True, True, drop("steps_applied"), "steps_applied"),
    ("moments of another length", False, True, change("m", torch.zeros(N - 1)), "m"),
    ("moments of another type", False, True, change("v", torch.zeros(N, dtype=torch.float64)), "v"),
    ("no moments", False, True, drop("m"), "m"),
    ("no step count", False, True, drop("t"), "t"),
]


@pytest.mark.parametrize("what,guard,ema,edit,field", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_load_state_dict_refuses_and_names_the_field(what, guard, ema, edit, field):
    ts = stub_step(guard=guard, ema=ema)
    sd = good_state(guard=guard, ema=ema)
    edit(sd)
    before = [None if t is None else t.clone() for t in (ts.m, ts.v, ts.ema)]
    with pytest.raises(T.StateError, match=r"^%s:" % field):
        ts.load_state_dict(sd)
    with pytest.raises(T.StateError, match=r"^%s:" % field):
        T.check_state(sd, own_of(ts))
    assert ts.t == 0, "a refused state changed the step"
    for a, b in zip((ts.m, ts.v, ts.ema), before):
        assert a is b or torch.equal(a, b), "a refused state changed the step"


def test_callers_own_settings_are_logged_not_refused(caplog):
    ts = stub_step()
    sd = good_state()
    sd.update(math="bf16x3", lr=1e-4, max_grad_norm=3.0)
    lines = T.check_state(sd, own_of(ts))
    assert sorted(l.split(":")[0] for l in lines) == ["lr", "math", "max_grad_norm"]
    with caplog.at_level("WARNING", logger=T.log.name):
        ts.load_state_dict(sd)
    assert ts.t == 7 and ts.math == "fp32" and ts.lr == 2e-4              # the step keeps ITS settings
    text = " ".join(r.getMessage() for r in caplog.records)
    assert "math" in text and "lr" in text and "max_grad_norm" in text


# ---------------------------------------------------------------------------------------------- the state file
def test_state_file_roundtrip_and_its_fields(tmp_path):
    ts = stub_step()
    ts.load_state_dict(good_state())
    path = str(tmp_path / "deep" / trainer.training_state_name("LFT", 2, 2))
    assert os.path.basename(path) == "LFT_2x2_2x_training_state.pth"
    extra = {"history": [0.5, 0.25], "last_metrics": [(30.0, 0.9)], "last_guard": [], "seed": 3, "global_batch": 4, "world": 2,
             "best": {"score": 31.5, "epoch": 2}}
    trainer.save_training_state(path, ts, 2, extra)
    assert os.listdir(os.path.dirname(path)) == [os.path.basename(path)]
    other = stub_step()
    got = trainer.load_training_state(path, other)
    assert got == dict(extra, epoch=2, file_version=trainer.STATE_FILE_VERSION)
    assert other.t == 7 and torch.equal(other.m, ts.m) and torch.equal(other.v, ts.v) and torch.equal(other.ema, ts.ema)
    with pytest.raises(ValueError, match="epoch"):
        trainer.save_training_state(path, ts, 2, {"epoch": 5})


FILE_REFUSALS = [
    ("not a dict", lambda st: [1, 2], "file_version"),
    ("no version", lambda st: {k: v for k, v in st.items() if k != "file_version"}, "file_version"),
    ("a newer file", lambda st: dict(st, file_version=trainer.STATE_FILE_VERSION + 1), "file_version"),
    ("no epoch", lambda st: {k: v for k, v in st.items() if k != "epoch"}, "epoch"),
    ("a negative epoch", lambda st: dict(st, epoch=-1), "epoch"),
    ("no optimizer state", lambda st: {k: v for k, v in st.items() if k != "train_step"}, "train_step"),
    ("optimizer state of another kind", lambda st: dict(st, train_step=[1]), "train_step"),
    ("optimizer state that does not fit", lambda st: dict(st, train_step=dict(st["train_step"], scale=4)), "scale"),
]


@pytest.mark.parametrize("what,edit,field", FILE_REFUSALS, ids=[r[0] for r in FILE_REFUSALS])
def test_file_loader_refuses_and_names_the_field(tmp_path, what, edit, field):
    state = {"file_version": trainer.STATE_FILE_VERSION, "epoch": 1, "train_step": good_state(), "history": [0.5]}
    path = str(tmp_path / "state.pth")
    torch.save(edit(state), path)
    ts = stub_step()
    with pytest.raises(T.StateError, match=r"^%s:" % field):
        trainer.load_training_state(path, ts)
    assert ts.t == 0 and not ts.m.any()


def test_a_failed_save_leaves_the_previous_file_and_no_temporary(tmp_path, monkeypatch):
    ts = stub_step()
    ts.load_state_dict(good_state())
    path = str(tmp_path / "state.pth")
    trainer.save_training_state(path, ts, 1, {"history": [0.5]})
    before = open(path, "rb").read()

    def dies_midway(obj, f, *a, **k):
        with open(f, "wb") as fh:                                           # half a file, as a killed process leaves it
            fh.write(b"half")
        raise OSError("disk full")

    monkeypatch.setattr(torch, "save", dies_midway)
    ts.t = 99
    with pytest.raises(OSError, match="disk full"):
        trainer.save_training_state(path, ts, 2, {"history": [0.5, 0.4]})
    monkeypatch.undo()
    assert open(path, "rb").read() == before
    assert os.listdir(str(tmp_path)) == ["state.pth"], "a temporary file was left behind"
    assert trainer.load_training_state(path, stub_step())["epoch"] == 1


# ---------------------------------------------------------------------------------------------- the EMA schedule
def test_ema_decay_schedule_follows_its_formula():
    for decay in (0.0, 0.5, 0.9, 0.999, 0.9999):
        d32 = float(np.float32(decay))                                      # what crosses the C ABI
        reached = None
        for t in range(1, 200000, 1 if decay < 0.9999 else 7):
            want = min(d32, (1.0 + t) / (10.0 + t))
            assert T.ema_decay_at(decay, True, t) == want
            if reached is None and want == d32:
                reached = t
            if reached is not None and t > reached + 3:
                break
        assert T.ema_decay_at(decay, False, 1) == d32 and T.ema_decay_at(decay, False, 10 ** 6) == d32
        # (1 + t) / (10 + t) >= d  <=>  t >= (10 d - 1) / (1 - d)
        bound = (10.0 * d32 - 1.0) / (1.0 - d32)
        assert reached is not None and abs(reached - max(1.0, bound)) <= (1 if decay < 0.9999 else 8), (decay, reached, bound)
    assert T.ema_decay_at(0.999, True, 1) == 2.0 / 11.0 and T.ema_decay_at(0.999, True, 2) == 3.0 / 12.0


def test_ema_decay_outside_its_range_is_refused_before_anything_is_built():
    for bad in (1.0, -0.1, 1.5, float("nan")):
        with pytest.raises(ValueError, match="ema_decay"):
            T.TrainStep(None, ema_decay=bad)


# ---------------------------------------------------------------------------------------------- the launcher's arguments
def launcher():
    spec = importlib.util.spec_from_file_location("train_dp_under_test", os.path.join(ROOT, "tools", "train_dp.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_resume_with_use_pre_pth_is_refused(capsys):
    L = launcher()
    with pytest.raises(SystemExit) as e:
        L.parse_args(["--resume", "auto", "--use_pre_pth"])
    assert e.value.code == 2 and "--use_pre_pth" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        L.parse_args(["--resume", "/some/state.pth", "--use_pre_pth"])
    args = L.parse_args([])                                                  # the defaults: everything new is off
    assert args.resume is None and not args.save_state and args.ema_decay is None and not args.no_ema_warmup and args.path_for_test is None


def test_resume_auto_takes_the_state_file_or_starts_fresh(tmp_path):
    L = launcher()
    args = L.parse_args(["--resume", "auto", "--path_log", str(tmp_path), "--angRes", "2", "--scale_factor", "2"])
    said = []
    assert L.resolve_resume(args, log=said.append) is None and len(said) == 1 and "starting fresh" in said[0]
    ckpt = L.checkpoint_dir(args)
    assert ckpt == os.path.join(str(tmp_path), "SR_2x2_2x", "LFT", "checkpoints")
    os.makedirs(ckpt)
    path = os.path.join(ckpt, "LFT_2x2_2x_training_state.pth")
    open(path, "wb").close()
    assert L.resolve_resume(args, log=said.append) == path and len(said) == 1
    explicit = L.parse_args(["--resume", "/elsewhere/state.pth"])
    assert L.resolve_resume(explicit) == "/elsewhere/state.pth"
    assert L.resolve_resume(L.parse_args([])) is None
