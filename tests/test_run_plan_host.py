"""The schedule of a run (csrc/mcpc_plan.h: plan_run, plan_hebbian) through mcpc_debug_run_plan -- no GPU.

`_model` is a transcription of the loop mcpc_run held before the schedule became data (commit 565feb4, csrc/mcpc_api.hip lines
1085-1240): where a call is cut at the accumulation window, how long a Hebbian segment is, when a stretch runs as cycles of the round
schedule and with which q, and which part of the spill ring a segment fills.  The library's plan is compared with it item for item
over a seeded sweep of (net, tuning, run shape), and held to the properties the executor and the ring rely on without the model.
`_heb_model` mirrors plan_hebbian of the same commit (lines 528-572): the split count of a flush never exceeds the one the slabs
are sized for.  `_flush_model` is a transcription of what flush_spill decided while it launched, before the flush became data too
(commit e752590, csrc/mcpc_api.hip lines 636-740): the kernel instantiation of every launch, its grid, first column and stream, the
reduction jobs and the text of mcpc_last_flush_plan.  The library's planned flushes (plan_flush) equal it launch for launch and
character for character over the same sweep and over directed shapes that reach every instantiation and every branch."""
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
    kn = dict(flush_tail=0, rr_qmax=100, dw_ksplit=0, heb_fp32=0, heb171=0, flush_streams=2)
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


def _heb_tiles(ne, na):
    """The tiling plan_hebbian gives a Linear of ne x na padded units: (wide, narrow_in, ra, te[2], n_mt[2], n_nt)."""
    et, at = ne // 16, na // 16
    wide = et >= 8 and at % 8 == 0 and (at <= 16 or at % 16 == 0)
    narrow_in = not wide and et == 16 and at in (1, 2, 4)
    ra, te, n_mt, n_nt = 0, [0, 0], [0, 0], 1
    if wide:
        ra = 2 if at >= 16 else 1
        n_nt = at // (8 * ra)
        if et <= 8:
            te, n_mt = [8, 0], [1, 0]
        elif et <= 16:
            te, n_mt = [16, 0], [1, 0]
        else:
            b17 = et % 16
            if et - 17 * b17 >= 0:
                te, n_mt = [17, 16], [b17, (et - 17 * b17) // 16]
            else:
                te, n_mt = [17, 0], [(et + 16) // 17, 0]
            if n_mt[0] == 0:
                te, n_mt = [te[1], 0], [n_mt[1], 0]
    elif narrow_in:
        ra, te, n_mt = 2, [at, 0], [1, 0]
    return wide, narrow_in, ra, te, n_mt, n_nt


def _heb_model(ne, na, rows, dw_ksplit=0):
    """(ksplit, rps, ksplit_cap) of plan_hebbian for a Linear of ne x na padded units and `rows` spilled rows."""
    KB = 32
    wide, narrow_in, _, _, n_mt, n_nt = _heb_tiles(ne, na)
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


# the <TE, RA, SWAPPED> instantiations of the tiled Hebbian kernels, in the order of csrc/mcpc_hebbian.h: MCPC_HEB_FORMS
HEB_FORMS = [(17, 2, 0), (17, 1, 0), (16, 2, 0), (16, 1, 0), (8, 2, 0), (8, 1, 0), (1, 2, 1), (2, 2, 1), (4, 2, 1)]
LAUNCH_FIELDS = ["family", "form", "te", "ra", "swapped", "n_mt", "n_nt", "col0", "stream", "wave_tiles"]


def _lins(p):
    """(out_pad, in_pad) of every Linear j >= 1 of an engine plan."""
    return list(zip(p["npad"][1:] + ([p["out_pad"]] if p["out_pad"] else []), p["npad"]))


def _flush_model(p, tuning, rows, two):
    """What flush_spill of commit e752590 (csrc/mcpc_api.hip lines 636-740, with plan_hebbian of csrc/mcpc_plan.h lines 939-983) launched
    for a flush of `rows` spilled rows on the engine plan `p`, decided as it decided them while launching.  `two`: its
    `aux3 != nullptr && stream == aux` -- ensure_spill (lines 578-592) created aux when the flushes overlap and aux3 when also
    flush_streams >= 2, and only an overlapped flush ran on aux.  Per Linear j >= 1: the launches as rows of LAUNCH_FIELDS without
    "form" (te, ra, swapped: the template arguments the if / else chains of lines 678-718 picked, their last `else` included), the
    text of mcpc_last_flush_plan, (sign, tr_cols, tr_ld) of its weight slab's reduction job; and the reduction launch's max_blocks."""
    kn = _knobs(tuning)
    fp32, heb171 = bool(kn["heb_fp32"]), bool(kn["heb171"])
    heb_name = "heb" if fp32 else "heb7"
    load = [0.0, 0.0]

    def next_stream(cost):                                   # greedy: the launch goes to the stream with less work queued
        k = 1 if two and load[1] < load[0] else 0
        load[k] += cost
        return k

    def name_launch(plan, kern, te, ra, sw, n_mt, n_nt):
        return plan + "%s%s<%d,%d%s>x%d" % ("+" if plan else "", kern, te, ra, ",T" if sw else "", n_mt) + ("*%d" % n_nt if n_nt > 1 else "")

    def chain(te, ra):                                       # lines 698-718, the same for both kernels once the re-split is taken out
        for t, r in ((17, 2), (16, 2), (8, 2)):
            if te == t and ra == 2:
                return t, r
        return (17, 1) if te == 17 else (16, 1) if te == 16 else (8, 1)

    launches, texts, reduce, max_blocks = [], [], [], 1
    L = len(p["npad"])
    for j, (ne, na) in enumerate(_lins(p), 1):
        wide, narrow_in, ra, te, n_mt, n_nt = _heb_tiles(ne, na)
        ksplit, rps, _ = _heb_model(ne, na, rows, kn["dw_ksplit"])
        mine, plan = [], ""
        if narrow_in:
            stream = next_stream(float(ne * na))
            plan = name_launch(plan, heb_name, te[0], 2, True, 1, 1)
            mine.append([heb_name, 1 if te[0] == 1 else 2 if te[0] == 2 else 4, 2, 1, 1, 1, 0, stream, 0])
        elif wide:
            col = 0
            for part in range(2):
                if n_mt[part] == 0:
                    continue
                stream = next_stream(float(n_mt[part] * te[part] * 16 * na))
                t = te[part]
                resplit = t == 17 and ra == 2 and not fp32 and heb171
                if not resplit:
                    plan = name_launch(plan, heb_name, t, ra, False, n_mt[part], n_nt)
                    mine.append([heb_name, *chain(t, ra), 0, n_mt[part], n_nt, col, stream, 0])
                else:
                    plan = name_launch(plan, heb_name, 17, 1, False, n_mt[part], 2 * n_nt)
                    mine.append([heb_name, 17, 1, 0, n_mt[part], 2 * n_nt, col, stream, 0])
                col += n_mt[part] * t * 16
        else:
            stream = next_stream(float(ne * na))
            wave_tiles = ((ne + 63) // 64) * ((na + 63) // 64)
            plan = "dw tiles=%d" % wave_tiles
            mine.append(["dw", 0, 0, 0, 0, 0, 0, stream, wave_tiles])
        launches.append(mine)
        texts.append(plan + " ksplit=%d rps=%d" % (ksplit, rps) + (" tm" if p["spill_tm"][j] else " rm"))
        reduce.append([-1 if j < L else 1, ne if narrow_in else 0, na if narrow_in else 0])
        max_blocks = max(max_blocks, min((ne * na + 255) // 256, 2048))
    return launches, texts, reduce, max_blocks


def _check_flushes(net, p, rp, seen=None):
    """Every flush of the run plan `rp` against _flush_model, launch for launch and character for character; every launch names the
    instantiation it runs (a valid index into HEB_FORMS whose entry is its te, ra, swapped -- nothing falls through to a default);
    no Linear's K-splits outgrow the slab plan_engine sized for it.  Returns the number of flushes checked."""
    assert rp["launch_fields"] == LAUNCH_FIELDS and rp["reduce_fields"] == ["sign", "tr_cols", "tr_ld"]
    kn = _knobs(net["tuning"])
    two = bool(rp["overlap"]) and kn["flush_streams"] >= 2
    lins = _lins(p)
    # the slabs: one region per Linear j >= 1, back to back
    off = 0
    for j, (slab_off, slab_floats, splits) in enumerate(p["slabs"]):
        if j == 0:
            assert (slab_off, slab_floats, splits) == (0, 0, 0)
            continue
        ne, na = lins[j - 1]
        assert slab_off == off and slab_floats == splits * (ne * na + ne), (net, j)
        assert splits == _heb_model(ne, na, p["half_slots"] * p["Bpad"], kn["dw_ksplit"])[2]
        off += slab_floats
    assert off == p["slab_floats"] and len(p["slabs"]) == len(lins) + 1
    models = {}
    for fl in rp["flushes"]:
        rows = fl["rows"]
        if rows not in models:
            models[rows] = _flush_model(p, net["tuning"], rows, two)
        launches, texts, reduce, max_blocks = models[rows]
        assert fl["two_streams"] == int(two) and fl["max_blocks"] == max_blocks and fl["reduce"] == reduce, (net, fl)
        assert fl["text"] == texts, (net, fl["text"], texts)
        assert [[l[:1] + l[2:] for l in lin] for lin in fl["launches"]] == launches, (net, fl["launches"], launches)
        for j, (lin, (ksplit, rps, cap)) in enumerate(zip(fl["launches"], fl["lin"]), 1):
            ne, na = lins[j - 1]
            assert ksplit * (ne * na + ne) <= p["slabs"][j][1], (net, j, ksplit)
            for l in map(lambda row: dict(zip(LAUNCH_FIELDS, row)), lin):
                assert l["stream"] in ((0, 1) if two else (0,)), (net, l)
                if l["family"] == "dw":
                    assert l["form"] == -1 and len(lin) == 1
                else:
                    assert 0 <= l["form"] < len(HEB_FORMS) and HEB_FORMS[l["form"]] == (l["te"], l["ra"], l["swapped"]), (net, l)
                    assert l["family"] == ("heb" if kn["heb_fp32"] else "heb7")
                if seen is not None:
                    seen.add((l["family"], l["form"]))
                    seen.add("stream %d" % l["stream"])
    return len(models)


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
    """plan_engine sizes a Linear's slabs by the `ksplit_cap` of a flush of a whole ring part; every flush of every run fits them."""
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


def test_the_library_plans_the_flushes_the_launcher_chose(sweep):
    """The planned flush of every Hebbian segment of the sweep is what flush_spill used to decide while launching."""
    n, seen = 0, set()
    for net, run, p, rp in sweep:
        assert len(rp["flushes"]) == sum(1 for it in rp["items"] if it[FIELDS.index("flush")])
        n += _check_flushes(net, p, rp, seen)
    families = {s[0] for s in seen if isinstance(s, tuple)}
    print("flush sweep: %d distinct flushes, launches seen %s" % (n, sorted(map(str, seen))))
    assert n >= 1000 and families == {"heb7", "dw"} and {"stream 0", "stream 1"} <= seen, (n, seen)


# Directed shapes: each row a net (latent sizes, read-out) whose Linears j >= 1 take the plans named behind it
FLUSH_NETS = [
    ([16, 256, 256], 272),            # 16->256 <1,2,T>; 256->256 <16,2>; 256->272 <17,2> (heb171=1: <17,1> x 2 activation groups)
    ([32, 256, 128, 128], 272),       # 32->256 <2,2,T>; 256->128 <8,2> (et <= 8); 128->128 <8,1>; 128->272 <17,1>
    ([64, 256, 128], 256),            # 64->256 <4,2,T>; 256->128 <8,2>; 128->256 <16,1>
    ([128, 256], 528),                # 256->528 = 17 + 16 tiles: two launches
    ([128, 256], 304),                # 19 tiles: a ragged group of 17 (2 x 17 > 19)
    ([128, 256], 240),                # 15 tiles on <16,2> (et <= 16)
    ([512, 256], 784),                # 512->256: an input of 32 tiles, two activation groups; 256->784 = 17 + 16 + 16
    ([32, 48, 100], 60),              # the streaming kernel
]
FLUSH_TUNINGS = [None, "heb_fp32=1", "heb171=1", "heb171=1,heb_fp32=1", "flush_streams=1", "no_overlap=1", "dw_ksplit=7", "dw_ksplit=7,heb_fp32=1"]


def test_directed_flush_shapes_reach_every_plan():
    """Every instantiation in both families, every branch of the tiling, the re-split, one and two streams, serial flushes and a forced
    split count -- each asserted as seen, so the sweep cannot shrink unnoticed.  A ring of three parts of 4 slots and a window of 10
    steps: segments of 4, 4 and 2 steps, two distinct flushes per run."""
    seen, hit = set(), set()
    run = dict(T=10, t_begin=0, n_steps=10, acc_begin=0, acc_end=10, update_x=1, xopt_kind=SGD, noise_mode=1, loss_kind=LOSS_BERNOULLI)
    for sizes, n_out in FLUSH_NETS:
        for extra in FLUSH_TUNINGS:
            net = dict(sizes=sizes, n_out=n_out, batch=64, tuning="wide=1,slot_cap=12" + ("," + extra if extra else ""))
            p, rp = plan(**net), run_plan(run=run, **net)
            kn = _knobs(net["tuning"])
            assert rp["overlap"] == int("no_overlap" not in net["tuning"])
            assert _check_flushes(net, p, rp, seen) == (2 if rp["overlap"] else 1)
            for fl in rp["flushes"]:
                streams = {l[LAUNCH_FIELDS.index("stream")] for lin in fl["launches"] for l in lin}
                if kn["flush_streams"] == 1 or not rp["overlap"]:
                    assert streams == {0} and not fl["two_streams"]
                    hit.add("flush_streams=1" if rp["overlap"] else "no_overlap=1")
                for (ne, na), lin, text, (_, _, cap) in zip(_lins(p), fl["launches"], fl["text"], fl["lin"]):
                    rows = [dict(zip(LAUNCH_FIELDS, l)) for l in lin]
                    et = ne // 16
                    if [(l["te"], l["n_mt"]) for l in rows] == [(17, et % 16), (16, (et - 17 * (et % 16)) // 16)]:
                        hit.add("17 + 16")
                    if len(rows) == 1 and rows[0]["te"] == 17 and rows[0]["n_mt"] * 17 > et:
                        hit.add("ragged 17")
                    if rows[0]["te"] == 8 and et <= 8:
                        hit.add("et <= 8")
                    if rows[0]["te"] == 16 and 8 < et <= 16 and not rows[0]["swapped"]:
                        hit.add("et <= 16")
                    if rows[0]["family"] != "dw" and not rows[0]["swapped"] and na // 16 > 16 and rows[0]["n_nt"] == na // 256:
                        hit.add("input wider than 16 tiles")
                    if rows[0]["swapped"]:
                        hit.add("swapped %d" % (na // 16))
                        assert (rows[0]["te"], rows[0]["n_mt"], rows[0]["n_nt"], rows[0]["col0"]) == (na // 16, 1, 1, 0)
                    if rows[0]["family"] == "dw":
                        hit.add("dw")
                    if kn["heb171"] and not kn["heb_fp32"] and text.startswith("heb7<17,1>x1*2 "):
                        assert na == 256 and (rows[0]["te"], rows[0]["ra"], rows[0]["n_nt"]) == (17, 1, 2)      # no flag: the launch itself
                        hit.add("heb171=1")
                    if kn["heb171"] and kn["heb_fp32"] and text.startswith("heb<17,2>x1 "):
                        hit.add("heb171=1 leaves the fp32 form alone")
                    if kn["dw_ksplit"] == 7 and rows[0]["family"] != "dw" and cap == 7:       # (the splits asked for; _check_flushes holds ksplit, rps to them)
                        hit.add("dw_ksplit=7")
    want_hit = {"17 + 16", "ragged 17", "et <= 8", "et <= 16", "input wider than 16 tiles", "swapped 1", "swapped 2", "swapped 4", "dw",
                "heb171=1", "heb171=1 leaves the fp32 form alone", "flush_streams=1", "no_overlap=1", "dw_ksplit=7"}
    print("directed flush shapes: %s" % sorted(hit))
    assert hit == want_hit, (want_hit - hit, hit - want_hit)
    want_seen = {(fam, i) for fam in ("heb7", "heb") for i in range(len(HEB_FORMS))} | {("dw", -1), "stream 0", "stream 1"}
    assert seen == want_seen, (want_seen - seen, seen - want_seen)


def test_the_learning_calls_flush_text():
    """cfg-M's learning call: 784 x 256 as one group of 17 tiles and two of 16, 256 x 256 on <16,2>, 256 x 32 with the operands swapped."""
    run = dict(T=5000, t_begin=0, n_steps=5000, acc_begin=1000, acc_end=5000, update_x=1, xopt_kind=SGD, noise_mode=1, loss_kind=LOSS_BERNOULLI)
    rp = run_plan(run=run, **CFG_M)
    for fl in rp["flushes"]:
        ks = [k for k, _, _ in fl["lin"]]
        rps = [r for _, r, _ in fl["lin"]]
        assert fl["text"] == ["heb7<2,2,T>x1 ksplit=%d rps=%d tm" % (ks[0], rps[0]), "heb7<16,2>x1 ksplit=%d rps=%d tm" % (ks[1], rps[1]),
                              "heb7<17,2>x1+heb7<16,2>x2 ksplit=%d rps=%d tm" % (ks[2], rps[2])]
        assert fl["two_streams"] == 1 and [[l[LAUNCH_FIELDS.index("stream")] for l in lin] for lin in fl["launches"]] == [[0], [1], [0, 1]]


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
