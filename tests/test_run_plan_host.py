"""The schedule of a run (csrc/mcpc_plan.h: plan_run, plan_hebbian) through mcpc_debug_run_plan -- no GPU.

`_model` is a transcription of the loop mcpc_run held before the schedule became data (commit 565feb4, csrc/mcpc_api.hip lines
1085-1240): where a call is cut at the accumulation window, how long a Hebbian segment is, when a stretch runs as cycles of the round
schedule and with which q, and which part of the spill ring a segment fills.  The library's plan is compared with it item for item
over a seeded sweep of (net, tuning, run shape), and held to the properties the executor and the ring rely on without the model.
`_heb_model` mirrors plan_hebbian of the same commit (lines 528-572): the split count of a flush never exceeds the one the slabs
are sized for."""
import random

import pytest

from tests.plan_util import plan, run_plan

ENOMEM = -3
GEN_BITS = (1 << 24) - 2
FIELDS = ["t0", "n", "q", "acc", "part", "slot0", "flush"]
CFG_M = dict(sizes=[30, 256, 256], n_out=784, batch=6000)
SGD, ADAM = 0, 1
LOSS_NONE, LOSS_BERNOULLI = 0, 2


def _knobs(tuning):
    kn = dict(flush_tail=0, rr_qmax=100, dw_ksplit=0)
    for item in (tuning or "").split(","):
        if "=" in item and item.split("=")[0] in kn:
            kn[item.split("=")[0]] = int(item.split("=")[1])
    return kn


def _model(p, tuning, run):
    """Rows of FIELDS for `run` on the engine plan `p` (mcpc_debug_plan), as the loop of 565feb4 issued its launches."""
    kn = _knobs(tuning)
    slots, half_slots = p["slots"], p["half_slots"]
    rr_k, rr_m = p["rounds"]["k"], p["rounds"]["m"]
    acc_b, acc_e = max(run["acc_begin"], 0), min(run["acc_end"], run["T"])
    t, end = run["t_begin"], run["t_begin"] + run["n_steps"]
    overlap = half_slots < slots                     # (what `e->aux != nullptr` is once ensure_spill has run)
    half, n_parts = 0, max(1, slots // max(1, half_slots))
    rr_ok = bool(p["rounds"]["on"]) and bool(run["update_x"])
    gen_cap = GEN_BITS // max(p["main"]["n_phases"], p["unified"]["plan"]["n_phases"], 1)
    items = []
    while t < end:
        in_acc = acc_b <= t < acc_e
        if in_acc:
            rem = min(end, acc_e) - t
            n = min(rem, half_slots)
            tail = kn["flush_tail"]
            if overlap and tail > 0 and rem <= half_slots and rem >= 2 * tail and min(end, acc_e) == acc_e:
                n = rem - tail
        else:
            n = (min(end, acc_b) if t < acc_b else end) - t
        n = min(n, gen_cap)
        rr_q = 0
        if rr_ok and in_acc:
            rr_q = n // rr_m
            if rr_q >= 1:
                n = rr_q * rr_m
        elif rr_ok:
            while n >= rr_m:
                q = min(max(1, kn["rr_qmax"]), n // rr_m)
                items.append([t, q * rr_m, q, 0, 0, 0, 0])
                t += q * rr_m
                n -= q * rr_m
            if n == 0:
                continue
        slot0 = half * half_slots if in_acc and overlap else 0
        items.append([t, n, rr_q, int(in_acc), half if in_acc and overlap else 0, slot0, int(in_acc)])
        if in_acc and overlap:
            half = (half + 1) % n_parts
        t += n
    return items


def _use_unified(p, tuning, run):
    """use_unified of 565feb4 (lines 894-906) on the plan's JSON; lean_ok needs Bpad x widest row < 2^32 bytes, true for every net here."""
    u = p["unified"]
    lean = "no_lean" not in (tuning or "")
    serves = (run["xopt_kind"] == SGD and run["noise_mode"] != 2) or (run["xopt_kind"] == ADAM and run["noise_mode"] == 0)
    has_head = p["out_pad"] > 0
    return int(bool(u["on"] and (u["prefer"] or (has_head and run["loss_kind"] == LOSS_NONE)) and p["form"] == "in-place"
                    and run["update_x"] and lean and serves))


def _heb_model(ne, na, rows, dw_ksplit=0):
    """(ksplit, rps, ksplit_cap) of plan_hebbian for a Linear of ne x na padded units and `rows` spilled rows."""
    KB = 32
    et, at = ne // 16, na // 16
    wide = et >= 8 and at % 8 == 0 and (at <= 16 or at % 16 == 0)
    narrow_in = not wide and et == 16 and at in (1, 2, 4)
    n_mt, n_nt = [0, 0], 1
    if wide:
        ra = 2 if at >= 16 else 1
        n_nt = at // (8 * ra)
        if et <= 16:
            n_mt = [1, 0]
        else:
            b17 = et % 16
            if et - 17 * b17 >= 0:
                n_mt = [b17, (et - 17 * b17) // 16]
            else:
                n_mt = [(et + 16) // 17, 0]
            if n_mt[0] == 0:
                n_mt = [n_mt[1], 0]
    elif narrow_in:
        n_mt = [1, 0]
    if wide or narrow_in:
        want = dw_ksplit if dw_ksplit > 0 else max(1, rows // (48 * KB))
        if dw_ksplit <= 0:
            cols = max(1, (n_mt[0] + n_mt[1]) * n_nt)
            want = max(want, min(rows // (8 * KB), (256 + cols - 1) // cols))
        want = min(want, max(1, rows // KB))
        rps = ((rows + want - 1) // want + KB - 1) // KB * KB
    else:
        wave_tiles = ((ne + 63) // 64) * ((na + 63) // 64)
        want = max(1, min(4096 // wave_tiles, rows // 64))
        rps = ((rows + want - 1) // want + 15) // 16 * 16
    return (rows + rps - 1) // rps, rps, want


# ---- the sweep ----------------------------------------------------------------------------------------------------------------------------------
def _window(rng, T, t_begin, n_steps):
    end = t_begin + n_steps
    kind = rng.choice(["empty", "never", "all", "before", "after", "inside", "inside", "inside", "tail"])
    if kind == "empty":
        return rng.randint(0, T), 0                                # acc_end <= acc_begin
    if kind == "never":
        return 0, 0
    if kind == "all":
        return 0, T
    if kind == "before":
        return -rng.randint(1, 50), rng.randint(t_begin + 1, T)   # starts before the call (and before t_begin)
    if kind == "after":
        return rng.randint(0, end - 1), T + rng.randint(1, 50)     # ends after T
    if kind == "tail":
        return rng.randint(t_begin, end - 1), T                    # the learning call: mixing, then sampling to the end
    a = rng.randint(t_begin, end - 1)
    return a, rng.randint(a + 1, end)


def _sweep(seed=20241019, count=2400):
    """Nets as in test_plan_host._sweep with widths up to 256; every knob that shapes a run; run shapes of every kind."""
    rng = random.Random(seed)
    for i in range(count):
        sizes = [min(256, int(round(256 ** rng.random()))) for _ in range(rng.randint(1, 4))]
        n_out = rng.choice([0, rng.randint(1, 1200), rng.randint(1, 1200)])
        n_cu = rng.choice([8, 20, 64, 256])
        ws = rng.choice([None, None, None, 0, 2, 2, 3, 4])
        knobs = [] if ws is None else ["ws=%d" % ws]
        if rng.random() < 0.3:
            knobs.append("no_overlap=1")
        if rng.random() < 0.6:
            knobs.append("ring_parts=%d" % rng.randint(2, 8))
        if rng.random() < 0.8:
            knobs.append("slot_cap=%d" % rng.choice([2, 3, 5, 6, 7, 12, 16, 33, 64, 100, 384]))
        if rng.random() < 0.5:
            knobs.append("flush_tail=%d" % rng.choice([0, 1, 2, 3, 5]))
        if rng.random() < 0.5:
            knobs.append("rr_qmax=%d" % rng.choice([1, 5, 100]))
        if rng.random() < 0.5:
            knobs.append("cu_slack=%d" % rng.randint(0, n_cu - 1))
        if rng.random() < 0.15:
            knobs.append("dw_ksplit=7")
        if ws != 4:                                                 # (ws=4 refuses the knobs of the LDS-resident kernels)
            if rng.random() < 0.2:
                knobs.append("rr=0")
            if rng.random() < 0.1:
                knobs.append("no_lean=1")
        # more 16-chain units than CUs in two cases of three, so that the round schedule is planned with few units as well
        batch = rng.randint(16 * n_cu + 1, 48 * n_cu) if rng.random() < 0.67 else rng.randint(1, 16 * n_cu)
        T = rng.choice([1, 2, 7, 40, 41, 93, 300, 1000, 5000])
        t_begin = rng.choice([0, 0, rng.randint(0, T - 1)])
        n_steps = rng.choice([T - t_begin, rng.randint(1, T - t_begin)])
        acc_begin, acc_end = _window(rng, T, t_begin, n_steps)
        xopt = rng.choice([SGD, SGD, ADAM])
        run = dict(T=T, t_begin=t_begin, n_steps=n_steps, acc_begin=acc_begin, acc_end=acc_end, update_x=int(rng.random() < 0.85),
                   xopt_kind=xopt, noise_mode=0 if xopt == ADAM else rng.choice([0, 1, 2]),
                   loss_kind=LOSS_NONE if n_out == 0 else rng.choice([LOSS_NONE, 1, LOSS_BERNOULLI]))
        yield dict(sizes=sizes, n_out=n_out, batch=batch, n_cu=n_cu, tuning=",".join(knobs) or None), run
    # one run long enough for the 24-bit generation of the row-exponent words to cut it (only the plan is computed)
    yield (dict(sizes=[16, 16], n_out=16, batch=16 * 21, n_cu=20, tuning="slot_cap=6"),
           dict(T=6_000_000, t_begin=0, n_steps=6_000_000, acc_begin=5_999_900, acc_end=6_000_000, update_x=1, xopt_kind=SGD, noise_mode=1,
                loss_kind=LOSS_BERNOULLI))
    yield (dict(sizes=[16, 16], n_out=16, batch=64, n_cu=256, tuning=None),
           dict(T=4_000_000, t_begin=100, n_steps=3_999_900, acc_begin=0, acc_end=0, update_x=0, xopt_kind=SGD, noise_mode=0,
                loss_kind=LOSS_BERNOULLI))


@pytest.fixture(scope="module")
def sweep():
    """[(net, run, engine plan, run plan)] of every case the planner accepts, computed once; the refusals are counted, none skipped."""
    from montecarlopredictivecoding_amd import _lib
    cases, refused, total = [], 0, 0
    plans = {}
    for net, run in _sweep():
        total += 1
        try:
            rp = run_plan(run=run, **net)
        except _lib.MCPCError as exc:
            assert exc.code == ENOMEM, (net, run, str(exc))        # only plan_engine's refusal of a net no LDS plan holds
            refused += 1
            continue
        key = repr(net)
        if key not in plans:
            plans[key] = plan(**net)
        assert rp["fields"] == FIELDS
        cases.append((net, run, plans[key], rp))
    assert total >= 2000 and refused <= total // 4, (total, refused)
    return cases


def test_the_library_plans_what_the_loop_did(sweep):
    forms, unified = set(), set()
    hit = dict(overlapped=0, serial=0, flush_tail=0, cycle_inside=0, cycle_outside=0, plain_remainder=0, generation_cap=0, ring_wraps=0)
    for net, run, p, rp in sweep:
        want = _model(p, net["tuning"], run)
        assert rp["items"] == want, (net, run, rp["items"][:6], want[:6])
        acc_b, acc_e = max(run["acc_begin"], 0), min(run["acc_end"], run["T"])
        end = run["t_begin"] + run["n_steps"]
        accumulates = acc_b < acc_e and run["t_begin"] < acc_e and end > acc_b
        assert rp["accumulates"] == int(accumulates) and rp["overlap"] == int(p["half_slots"] < p["slots"])
        assert rp["n_parts"] == max(1, p["slots"] // max(1, p["half_slots"]))
        assert rp["unified"] == _use_unified(p, net["tuning"], run), (net, run)
        assert rp["lean_ok"] == int("no_lean" not in (net["tuning"] or ""))
        forms.add(p["form"]); unified.add(rp["unified"])
        # what the sweep reached
        kn = _knobs(net["tuning"])
        gen_cap = GEN_BITS // max(p["main"]["n_phases"], p["unified"]["plan"]["n_phases"], 1)
        rows = [dict(zip(FIELDS, it)) for it in rp["items"]]
        acc = [k for k in rows if k["acc"]]
        if acc:
            hit["overlapped" if rp["overlap"] else "serial"] += 1
            hit["ring_wraps"] += int(rp["overlap"] and len(acc) > rp["n_parts"])
            last = acc[-1]
            # a stretch's last segment, cut short so that its flush (which nothing overlaps) is short
            hit["flush_tail"] += int(rp["overlap"] and kn["flush_tail"] > 0 and len(acc) >= 2 and last["t0"] + last["n"] == acc_e
                                     and acc[-2]["t0"] + acc[-2]["n"] == last["t0"] and last["n"] == kn["flush_tail"]
                                     and acc[-2]["n"] + last["n"] <= p["half_slots"])
        hit["cycle_inside"] += int(any(k["q"] and k["acc"] for k in rows))
        hit["cycle_outside"] += int(any(k["q"] and not k["acc"] for k in rows))
        hit["plain_remainder"] += int(p["rounds"]["on"] and run["update_x"] and any(not k["q"] for k in rows))
        hit["generation_cap"] += int(any(k["n"] == gen_cap for k in rows))
    print("run-plan sweep of %d cases: %s" % (len(sweep), hit))
    assert all(v >= (1 if k == "generation_cap" else 10) for k, v in hit.items()), hit
    assert forms == {"in-place", "barrier", "layer-wise"} and unified == {0, 1}


def test_every_run_plan_is_sound(sweep):
    for net, run, p, rp in sweep:
        rows = [dict(zip(FIELDS, it)) for it in rp["items"]]
        slots, half_slots, rr = p["slots"], p["half_slots"], p["rounds"]
        acc_b, acc_e = max(run["acc_begin"], 0), min(run["acc_end"], run["T"])
        # the items tile [t_begin, t_begin + n_steps) in order
        t = run["t_begin"]
        for k in rows:
            assert k["t0"] == t and k["n"] >= 1, (net, run, k)
            t += k["n"]
        assert t == run["t_begin"] + run["n_steps"]
        for k in rows:
            inside = [acc_b <= s < acc_e for s in (k["t0"], k["t0"] + k["n"] - 1)]
            assert inside[0] == inside[1] == bool(k["acc"]), (net, run, k)          # wholly on one side of the window
            assert k["flush"] == k["acc"]
            if k["acc"]:
                assert k["n"] <= half_slots and k["slot0"] + k["n"] <= slots and k["slot0"] == k["part"] * half_slots, (net, run, k)
            else:
                assert k["part"] == 0 and k["slot0"] == 0
            if k["q"]:
                assert rr["on"] and run["update_x"] and k["q"] >= 1 and k["n"] == rr["m"] * k["q"], (net, run, k)
                if not k["acc"]:
                    assert k["q"] <= max(1, _knobs(net["tuning"])["rr_qmax"])
        # ring parts: 0, 1, .. n_parts - 1, 0, .. when flushes overlap (a part is reused after n_parts - 1 other segments), 0 when serial
        parts = [k["part"] for k in rows if k["acc"]]
        if rp["overlap"]:
            assert rp["n_parts"] >= 2 and parts == [i % rp["n_parts"] for i in range(len(parts))], (net, run, parts[:10])
        else:
            assert rp["n_parts"] == 1 and not any(parts)


def test_no_flush_needs_more_splits_than_the_slabs_hold(sweep):
    """ensure_spill sizes a Linear's slabs by the `ksplit_cap` of a flush of a whole ring part; every flush of every run fits them."""
    n = 0
    for net, run, p, rp in sweep:
        flushing = [it for it in rp["items"] if it[FIELDS.index("flush")]]
        assert len(rp["flushes"]) == len(flushing)
        lins = list(zip(p["npad"][1:] + ([p["out_pad"]] if p["out_pad"] else []), p["npad"]))      # (out_pad, in_pad) of Linear j >= 1
        dwk = _knobs(net["tuning"])["dw_ksplit"]
        for it, fl in zip(flushing, rp["flushes"]):
            assert fl["rows"] == it[1] * p["Bpad"] and len(fl["lin"]) == len(lins)
            for (ne, na), (ksplit, rps, cap) in zip(lins, fl["lin"]):
                assert 1 <= ksplit <= cap, (net, run, it, ne, na, ksplit, cap)
                assert ksplit * rps >= fl["rows"]
                assert (ksplit, rps) == _heb_model(ne, na, fl["rows"], dwk)[:2]
                assert cap == _heb_model(ne, na, p["half_slots"] * p["Bpad"], dwk)[2]
                n += 1
    assert n >= 10000, n


@pytest.mark.parametrize("dw_ksplit", [0, 7])
def test_split_count_never_exceeds_that_of_a_whole_ring_part(dw_ksplit):
    """Directly: flushes of s = 1 .. half_slots slots of Bpad rows, for seeded Linear shapes (through a net of one hidden layer and a
    read-out, whose two Linears j >= 1 have those shapes)."""
    rng = random.Random(7 + dw_ksplit)
    checked = 0
    for _ in range(150):
        in_pad, out_pad = 16 * rng.randint(1, 16), 16 * rng.randint(1, 75)
        batch = 16 * rng.randint(1, 300)
        half = rng.choice([1, 2, 3, 8, 24, 64, 128])
        tuning = "rr=0,no_overlap=1,slot_cap=%d" % max(half, 2) + (",dw_ksplit=%d" % dw_ksplit if dw_ksplit else "")
        net = dict(sizes=[16, in_pad], n_out=out_pad, batch=batch, tuning=tuning, spill_budget_bytes=1 << 50)
        p = plan(**net)
        half = p["half_slots"]
        run = dict(t_begin=0, acc_begin=0, update_x=1, xopt_kind=SGD, noise_mode=1, loss_kind=LOSS_BERNOULLI)
        # one call per segment length s: a window of s steps is one serial segment of s slots
        for s in range(1, half + 1):
            rp = run_plan(run=dict(run, T=s, n_steps=s, acc_end=s), **net)
            (fl,) = rp["flushes"]
            assert fl["rows"] == s * p["Bpad"]
            for (ne, na), (ksplit, rps, cap) in zip([(in_pad, 16), (out_pad, in_pad)], fl["lin"]):
                assert ksplit <= cap and (ksplit, rps, cap) == (_heb_model(ne, na, s * p["Bpad"], dw_ksplit)[:2]
                                                                + _heb_model(ne, na, half * p["Bpad"], dw_ksplit)[2:]), (net, s)
                checked += 1
    assert checked >= 300


def test_split_count_invariant_of_the_mirror():
    """The property plan_hebbian had before it moved (dw_ksplit = 0, the default): 98 000 (shape, Bpad, part, slots) cases."""
    rng = random.Random(1)
    n = 0
    for _ in range(3000):
        ne, na = 16 * rng.randint(1, 75), 16 * rng.randint(1, 40)
        Bpad, half = 32 * rng.randint(1, 300), rng.choice([1, 2, 3, 8, 24, 64, 128])
        cap = _heb_model(ne, na, half * Bpad)[2]
        for s in range(1, half + 1):
            assert _heb_model(ne, na, s * Bpad)[0] <= cap, (ne, na, Bpad, half, s)
            n += 1
    assert n >= 98000


# ---- known answers ----------------------------------------------------------------------------------------------------------------------------
def test_the_benchmarks_learning_call():
    """6000 chains of 30-256-256 -> 784 on 256 CUs, T = 5000 with Hebbian sums over [1000, 5000): 375 units in cycles of k = 3
    launches, every unit in m = 2; the mixing stretch in cycles of 2 x 100 steps, the window in segments of one cycle of 2 x 64 steps
    (a ring part holds 128 slots) through parts 0, 1, 2, 0, ..; the last 32 steps are a cycle of 2 x 16."""
    p = plan(**CFG_M)
    assert (p["rounds"]["k"], p["rounds"]["m"], p["slots"], p["half_slots"]) == (3, 2, 384, 128)
    run = dict(T=5000, t_begin=0, n_steps=5000, acc_begin=1000, acc_end=5000, update_x=1, xopt_kind=SGD, noise_mode=1, loss_kind=LOSS_BERNOULLI)
    rp = run_plan(run=run, **CFG_M)
    assert (rp["unified"], rp["accumulates"], rp["lean_ok"], rp["overlap"], rp["n_parts"]) == (0, 1, 1, 1, 3)
    want = [[200 * i, 200, 100, 0, 0, 0, 0] for i in range(5)]
    want += [[1000 + 128 * i, 128, 64, 1, i % 3, 128 * (i % 3), 1] for i in range(31)]
    want += [[4968, 32, 16, 1, 31 % 3, 128 * (31 % 3), 1]]
    assert rp["items"] == want
    assert [fl["rows"] for fl in rp["flushes"]] == [128 * 6016] * 31 + [32 * 6016]
    # a zero-loss call of the same engine runs on the unified-wave kernel, gradients-only and injected-noise runs never do
    assert run_plan(run=dict(run, loss_kind=LOSS_NONE), **CFG_M)["unified"] == 1
    assert run_plan(run=dict(run, loss_kind=LOSS_NONE, update_x=0), **CFG_M)["unified"] == 0
    assert run_plan(run=dict(run, loss_kind=LOSS_NONE, noise_mode=2), **CFG_M)["unified"] == 0


def test_a_bad_step_range_is_refused_as_mcpc_run_refuses_it():
    from montecarlopredictivecoding_amd import _lib
    run = dict(T=10, t_begin=0, n_steps=10, acc_begin=0, acc_end=0, update_x=1, xopt_kind=SGD, noise_mode=0, loss_kind=LOSS_NONE)
    for bad in (dict(T=0), dict(t_begin=-1), dict(n_steps=0), dict(t_begin=5, n_steps=6)):
        with pytest.raises(_lib.MCPCError) as exc:
            run_plan(run=dict(run, **bad), sizes=[16], n_out=0, batch=16)
        assert exc.value.code == -1 and "bad step range" in str(exc.value)
