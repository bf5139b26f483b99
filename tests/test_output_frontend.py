"""CPU tests of the output front end (climaseaice.jl_amd/output.py) on the NumPy stand-in recorder of tests/output_ref.py: schedules,
averaging weights, aligned_time_step, the growable NPY files, load_output of a tiled run, slot handling."""
import json
import os
from collections import OrderedDict
from fractions import Fraction
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import climaseaice_jl_amd as csi
import output_ref as ref
from climaseaice_jl_amd.output import GrowableNpy

LOCS = {"u": (csi.Face, csi.Center), "v": (csi.Center, csi.Face), "h": (csi.Center, csi.Center), "aice": (csi.Center, csi.Center)}


def clock_at(time=0.0, iteration=0):
    return SimpleNamespace(time=time, iteration=iteration)


def run_schedule(s, dts, t0=0.0):
    """Drive a schedule over steps dts: (initial record?, [(iteration, end time, actions)])."""
    clock = clock_at(t0)
    s.attach(clock)
    first = s.initial(clock)
    log = []
    for dt in dts:
        clock.time += dt
        clock.iteration += 1
        log.append((clock.iteration, clock.time, s.after_step(clock, dt)))
    return first, log


# ---- schedules ------------------------------------------------------------------------------------------------------------------------
def test_iteration_interval():
    first, log = run_schedule(csi.IterationInterval(5), [1.0] * 12)
    assert first
    assert [it for it, _, a in log if a] == [5, 10]
    assert all(a == [("write", t)] for _, t, a in log if a)
    s = csi.IterationInterval(3)
    assert not s.initial(clock_at(0.0, 4)) and s.initial(clock_at(0.0, 6))
    with pytest.raises(ValueError):
        csi.IterationInterval(0)


def test_time_interval_with_steps_that_overshoot():
    # steps of 0.75 against an interval of 1: records after the steps that reach 1, 2, 3 (ends 1.5, 2.25, 3.0)
    first, log = run_schedule(csi.TimeInterval(1.0), [0.75] * 4)
    assert first and [t for _, t, a in log if a] == [1.5, 2.25, 3.0]
    # one step over several intervals: ONE record, and `next` lands beyond the clock
    s = csi.TimeInterval(1.0)
    first, log = run_schedule(s, [0.5, 3.75, 0.5, 0.5])
    assert [t for _, t, a in log if a] == [4.25, 5.25]
    assert s.next == 6.0
    # exactly on the interval
    first, log = run_schedule(csi.TimeInterval(0.5), [0.25] * 8)
    assert [it for it, _, a in log if a] == [2, 4, 6, 8]


def windows_of(log):
    """[(record time, [weights])] of an averaged schedule's log"""
    out, cur = [], []
    for _, _, actions in log:
        for kind, v in actions:
            if kind == "accumulate":
                cur.append(v)
            else:
                out.append((v, cur))
                cur = []
    return out, cur


def exact_sum(ws):
    return sum(Fraction(w) for w in ws)


def test_averaged_weights_window_equals_interval_variable_dt():
    """Dyadic steps: every overlap is exact, so the weights of a window sum to the window exactly."""
    dts = [0.25, 0.5, 0.125, 0.375, 0.75, 0.25, 0.5, 0.25, 1.0]         # ends .25 .75 .875 1.25 2.0 2.25 2.75 3.0 4.0
    first, log = run_schedule(csi.AveragedTimeInterval(1.0), dts)
    assert not first
    wins, rest = windows_of(log)
    assert [t for t, _ in wins] == [1.0, 2.0, 3.0, 4.0] and rest == []
    assert wins[0][1] == [0.25, 0.5, 0.125, 0.125]                      # the step (0.875, 1.25] is cut at t_out = 1 ...
    assert wins[1][1] == [0.25, 0.75]                                   # ... and its rest opens the next window
    assert all(exact_sum(w) == 1 for _, w in wins)


def test_averaged_weights_window_starts_inside_a_step():
    """window < interval: the window (t_out - window, t_out] starts inside a step, which enters with the overlap only; steps before
    it are skipped."""
    s = csi.AveragedTimeInterval(2.0, window=0.75)
    first, log = run_schedule(s, [0.5] * 8)                            # window 1: (1.25, 2.0], window 2: (3.25, 4.0]
    wins, rest = windows_of(log)
    assert [t for t, _ in wins] == [2.0, 4.0]
    assert wins[0][1] == [0.25, 0.5] and wins[1][1] == [0.25, 0.5]
    assert [it for it, _, a in log if not a] == [1, 2, 5, 6]            # zero-weight steps launch nothing
    assert all(exact_sum(w) == Fraction(3, 4) for _, w in wins)


def test_averaged_weights_step_over_several_intervals():
    first, log = run_schedule(csi.AveragedTimeInterval(1.0), [0.5, 2.75, 0.75])      # ends 0.5, 3.25, 4.0
    wins, rest = windows_of(log)
    assert [t for t, _ in wins] == [1.0, 2.0, 3.0, 4.0]
    assert [w for _, w in wins] == [[0.5, 0.5], [1.0], [1.0], [0.25, 0.75]]
    assert all(exact_sum(w) == 1 for _, w in wins)


def test_averaged_weights_sum_to_the_window_up_to_rounding():
    """Non-dyadic steps: each weight is one subtraction of doubles, so a window's sum is within n ulp of the window."""
    rng = np.random.default_rng(5)
    dts = list(rng.uniform(20.0, 140.0, 200))
    first, log = run_schedule(csi.AveragedTimeInterval(600.0, window=450.0), dts, t0=1000.0)
    wins, _ = windows_of(log)
    assert len(wins) >= 20
    for t, w in wins:
        assert abs(float(exact_sum(w)) - 450.0) <= len(w) * np.spacing(t + 600.0)


def fake_model(g, names=("u", "v", "h", "aice"), seed=0, mask=None):
    rng = np.random.default_rng(seed)
    fields = OrderedDict()
    for n in names:
        f = csi.Field(LOCS[n], g, None, n)
        f.data.copy_(torch.from_numpy(rng.standard_normal(tuple(f.data.shape))))
        fields[n] = f
    return SimpleNamespace(grid=g, clock=clock_at(), fields=fields, output_writers=OrderedDict(), mask_interior=mask)


def step(model, dt, evolve=None):
    for w in model.output_writers.values():
        w.begin(model)
    for k, f in enumerate(model.fields.values()):
        f.data.mul_(1.0 + 2.0 ** -(k + 3)).add_(2.0 ** -7)            # any change of state
    if evolve:
        evolve(model)
    model.clock.time += dt
    model.clock.iteration += 1
    for w in model.output_writers.values():
        w.after_step(model, dt)


def grid(topo=(csi.Bounded, csi.Bounded), size=(8, 6), halo=(2, 2)):
    return csi.RectilinearGrid(size, x=(0, size[0]), y=(0, size[1]), topology=topo, halo=halo)


def test_aligned_time_step(tmp_path):
    m = fake_model(grid())
    m.output_writers["snap"] = csi.OutputWriter(m, ["h"], csi.TimeInterval(1.0), str(tmp_path / "a"), recorder=ref.RefRecorder)
    m.output_writers["avg"] = csi.OutputWriter(m, ["h"], csi.AveragedTimeInterval(2.5), str(tmp_path / "b"), recorder=ref.RefRecorder)
    m.output_writers["it"] = csi.OutputWriter(m, ["h"], csi.IterationInterval(1), str(tmp_path / "c"), recorder=ref.RefRecorder)
    ends = []
    while m.clock.time < 5.0:
        dt = csi.aligned_time_step(m, 0.75)
        assert 0 < dt <= 0.75
        step(m, dt)
        ends.append(m.clock.time)
    assert ends == [0.75, 1.0, 1.75, 2.0, 2.5, 3.0, 3.75, 4.0, 4.75, 5.0]
    for w in m.output_writers.values():
        w.close()
    assert list(np.load(tmp_path / "a" / "time.npy")) == [0.0, 1.0, 2.0, 3.0, 4.0, 5.0]
    assert list(np.load(tmp_path / "b" / "time.npy")) == [2.5, 5.0]
    assert len(np.load(tmp_path / "c" / "iteration.npy")) == 11


# ---- files ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_files_are_valid_npy_after_every_record(tmp_path, dtype):
    g = grid()
    mask = np.ones((g.Ny, g.Nx), np.uint8)
    mask[0, :] = mask[:, -1] = 0
    m = fake_model(g, mask=mask)
    w = csi.OutputWriter(m, ["u", "v", "h", "aice"], csi.IterationInterval(1), str(tmp_path / "out"), dtype=dtype, mask=True,
                         fill_value=-999.0, slots=1, recorder=ref.RefRecorder)
    want = {n: [] for n in m.fields}
    for k in range(5):
        for n, f in m.fields.items():
            x = ref.interior(f.numpy(), g.Hx, g.Hy)
            want[n].append(ref.element(x, dtype, mask if n in ("h", "aice") else None, -999.0))
        w.write(m)
        step(m, 10.0)                         # (the record is the state at the call: it is drained after the state has moved on)
        w.flush()
        for n in m.fields:
            for mode in (None, "r"):
                a = np.load(tmp_path / "out" / f"{n}.npy", mmap_mode=mode)
                assert a.shape == (k + 1,) + want[n][0].shape and a.dtype == want[n][0].dtype
                assert ref.same_bits(np.asarray(a), np.stack(want[n][:k + 1])), (n, k, mode)
        assert list(np.load(tmp_path / "out" / "iteration.npy")) == list(range(k + 1))
        assert os.path.getsize(tmp_path / "out" / "h.npy") == 128 + (k + 1) * want["h"][0].nbytes
    w.close()
    assert (np.load(tmp_path / "out" / "h.npy")[:, 0, :] == -999.0).all() and not (np.load(tmp_path / "out" / "u.npy") == -999.0).any()
    meta = json.load(open(tmp_path / "out" / "meta.json"))
    assert [o["name"] for o in meta["outputs"]] == ["u", "v", "h", "aice"]
    assert meta["outputs"][0]["location"] == ["Face", "Center"] and meta["outputs"][0]["shape"] == [6, 9]
    assert meta["outputs"][2]["masked"] and meta["outputs"][2]["fill_value"] == -999.0 and not meta["outputs"][0]["masked"]
    assert meta["schedule"] == {"kind": "IterationInterval", "interval": 1} and meta["grid"]["Nx"] == 8 and meta["tile"] is None


def test_growable_npy_scalars_and_header(tmp_path):
    f = GrowableNpy(str(tmp_path / "t.npy"), "<f8", ())
    assert np.load(tmp_path / "t.npy").shape == (0,)
    for k in range(3):
        f.append(np.float64(k / 4))
    f.close()
    assert list(np.load(tmp_path / "t.npy")) == [0.0, 0.25, 0.5]
    assert open(tmp_path / "t.npy", "rb").read(128)[-1:] == b"\n" and os.path.getsize(tmp_path / "t.npy") == 128 + 24


def test_existing_directory_is_refused(tmp_path):
    m = fake_model(grid())
    d = str(tmp_path / "out")
    w = csi.OutputWriter(m, ["h"], csi.IterationInterval(1), d, recorder=ref.RefRecorder)
    w.write(m)
    w.close()
    with pytest.raises(FileExistsError):
        csi.OutputWriter(m, ["h"], csi.IterationInterval(1), d, recorder=ref.RefRecorder)
    w = csi.OutputWriter(m, ["h"], csi.IterationInterval(1), d, overwrite_existing=True, recorder=ref.RefRecorder)
    w.close()
    assert np.load(os.path.join(d, "h.npy")).shape == (0, 6, 8)


def test_outputs_are_resolved_by_name_or_by_field(tmp_path):
    m = fake_model(grid())
    with pytest.raises(ValueError, match="'sigma12'"):
        csi.OutputWriter(m, ["h", "sigma12"], csi.IterationInterval(1), str(tmp_path / "a"), recorder=ref.RefRecorder)
    stray = csi.Field(LOCS["h"], m.grid, None, "stray")
    with pytest.raises(ValueError, match="'thickness'"):
        csi.OutputWriter(m, {"thickness": stray}, csi.IterationInterval(1), str(tmp_path / "b"), recorder=ref.RefRecorder)
    with pytest.raises(ValueError, match="'time'"):
        csi.OutputWriter(m, {"time": m.fields["h"]}, csi.IterationInterval(1), str(tmp_path / "c"), recorder=ref.RefRecorder)
    with csi.OutputWriter(m, {"thickness": m.fields["h"]}, csi.IterationInterval(1), str(tmp_path / "d"), dtype="f64",
                          recorder=ref.RefRecorder) as w:
        w.write(m)
    got = csi.load_output(str(tmp_path / "d"))
    assert ref.same_bits(got["thickness"][0], ref.interior(m.fields["h"].numpy(), 2, 2))


def run_writers(tmp, slots, tag):
    m = fake_model(grid(), seed=4)
    m.output_writers["snap"] = csi.OutputWriter(m, ["u", "h"], csi.IterationInterval(2), os.path.join(tmp, tag, "snap"), slots=slots,
                                                recorder=ref.RefRecorder)
    m.output_writers["avg"] = csi.OutputWriter(m, ["v", "aice"], csi.AveragedTimeInterval(3.0, window=2.0),
                                               os.path.join(tmp, tag, "avg"), dtype="f64", slots=slots, recorder=ref.RefRecorder)
    for dt in [0.5, 1.0, 0.75, 0.75, 1.5, 0.5, 1.0, 1.0, 2.0]:
        step(m, dt)
    for w in m.output_writers.values():
        w.close()
    return {k: csi.load_output(os.path.join(tmp, tag, k)) for k in ("snap", "avg")}


def test_one_slot_and_three_slots_write_the_same_files(tmp_path):
    a, b = run_writers(str(tmp_path), 1, "one"), run_writers(str(tmp_path), 3, "three")
    assert list(a["snap"]["iteration"]) == [0, 2, 4, 6, 8] and list(a["avg"]["time"]) == [3.0, 6.0, 9.0]
    for k in a:
        assert sorted(a[k]) == sorted(b[k])
        for n in a[k]:
            assert ref.same_bits(a[k][n], b[k][n]), (k, n)
    for sub in ("snap", "avg"):
        for name in os.listdir(tmp_path / "one" / sub):
            assert open(tmp_path / "one" / sub / name, "rb").read() == open(tmp_path / "three" / sub / name, "rb").read(), (sub, name)


def test_averaged_records_are_the_restated_average(tmp_path):
    m = fake_model(grid(), names=("h",), seed=9)
    m.output_writers["avg"] = csi.OutputWriter(m, ["h"], csi.AveragedTimeInterval(1.0), str(tmp_path / "avg"), dtype="f64",
                                               recorder=ref.RefRecorder)
    states, dts = [], [0.25, 0.5, 0.125, 0.375, 0.75]
    for dt in dts:
        step(m, dt)
        states.append(ref.interior(m.fields["h"].numpy(), 2, 2).copy())
    m.output_writers["avg"].close()
    got = csi.load_output(str(tmp_path / "avg"))
    assert list(got["time"]) == [1.0, 2.0]
    assert ref.same_bits(got["h"][0], ref.averaged(states[:4], [0.25, 0.5, 0.125, 0.125]))
    assert ref.same_bits(got["h"][1], ref.averaged(states[3:5], [0.25, 0.75]))


def test_load_output_reassembles_a_2x2_tiling(tmp_path):
    """Bounded in x and y: the easternmost / northernmost tiles carry the extra face of u / v."""
    G = grid(size=(8, 6))
    whole = fake_model(G, seed=11)
    tiles = []
    for rank in range(4):
        t = csi.TileGrid(G, 2, 2, rank % 2, rank // 2)
        tm = fake_model(t, seed=rank)
        for n, f in tm.fields.items():
            src = ref.interior(whole.fields[n].numpy(), G.Hx, G.Hy)
            f.interior().copy_(torch.from_numpy(t.local_interior(src, *LOCS[n])))
        tm.output_writers["w"] = csi.OutputWriter(tm, ["u", "v", "h", "aice"], csi.IterationInterval(1), str(tmp_path / "tiled"),
                                                  dtype="f64", recorder=ref.RefRecorder)
        tiles.append(tm)
    whole.output_writers["w"] = csi.OutputWriter(whole, ["u", "v", "h", "aice"], csi.IterationInterval(1), str(tmp_path / "whole"),
                                                 dtype="f64", recorder=ref.RefRecorder)
    for _ in range(2):
        for m in tiles + [whole]:
            step(m, 1.0)                      # (the same point-wise change of state everywhere)
    for m in tiles + [whole]:
        m.output_writers["w"].close()
    assert sorted(os.listdir(tmp_path / "tiled")) == ["rank_0", "rank_1", "rank_2", "rank_3"]
    meta = json.load(open(tmp_path / "tiled" / "rank_3" / "meta.json"))
    assert meta["tile"]["rank"] == 3 and meta["tile"]["partition"] == [2, 2] and meta["outputs"][0]["offset"] == [4, 3]
    assert meta["outputs"][0]["shape"] == [3, 5] and meta["outputs"][1]["shape"] == [4, 4]
    a, b = csi.load_output(str(tmp_path / "tiled")), csi.load_output(str(tmp_path / "whole"))
    assert a["u"].shape == (3, 6, 9) and a["v"].shape == (3, 7, 8)
    for n in b:
        assert ref.same_bits(a[n], b[n]), n
