"""The planner of the depth-2 / depth-3 kernels (nsol_amd/csrc/nsol_pdk_plan.hpp) on the
CPU: tests/host/pdk_plan_check.cpp, built with the host compiler alone -- once plain, once
with the address and undefined-behaviour sanitizers -- and run as a child process.  No GPU,
no library.

The candidate lists and plan lists of a fixed set of shapes and knobs are pinned by
tests/pdk_plan_lists.json (the program's output before the list rules were folded into
one); the tuner's sampling state machine is replayed with synthetic times."""
import json
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "tests", "host", "pdk_plan_check.cpp")
LISTS = os.path.join(ROOT, "tests", "pdk_plan_lists.json")
BUILDS = {"plain": [], "sanitized": ["-g", "-fsanitize=address,undefined",
                                     "-fno-sanitize-recover=all"]}
# footprint rows a tiling loses to overlap, by form; per list kind the model's best that get
# on a list per workgroup size (ListRule::best in the header)
LOST = {"unshifted": 4, "shifted": 5}
BEST = {"short": 1, "shifted": 3, "full": 5}


def _clangxx():
    """The clang++ that hipcc drives."""
    roots = [os.environ.get("ROCM_PATH"), "/opt/rocm"]
    hipcc = shutil.which("hipcc")
    if hipcc:
        roots.append(os.path.dirname(os.path.dirname(os.path.realpath(hipcc))))
    for root in filter(None, roots):
        for sub in ("llvm/bin", "lib/llvm/bin"):
            exe = os.path.join(root, sub, "clang++")
            if os.path.exists(exe):
                return exe
    return None


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    cxx = _clangxx()
    if cxx is None:
        pytest.skip("ROCm's clang++ not available")
    out = {}
    for name, extra in BUILDS.items():
        exe = tmp_path_factory.mktemp("pdk_plan") / ("pdk_plan_check_" + name)
        subprocess.run([cxx, "-std=c++17", "-ffp-contract=off", "-O1"] + extra +
                       [SOURCE, "-o", str(exe)], check=True)
        out[name] = str(exe)
    return out


@pytest.fixture(scope="module", params=list(BUILDS))
def exe(request, programs):
    return programs[request.param]


@pytest.fixture(scope="module")
def cases():
    with open(LISTS) as f:
        return {c["case"]: c for c in json.load(f)}


# ---- the lists

def test_lists_are_the_committed_ones(exe):
    got = subprocess.run([exe], check=True, stdout=subprocess.PIPE).stdout
    with open(LISTS, "rb") as f:
        assert got == f.read()


def test_512_cubed_ranks_the_trimmed_twin_of_12_4_first(cases):
    """the twin of 12 : 4 with 16 valid rows (nty = 32: four tile rows
    per XCD) ranks first for both forms -- 21 footprint rows in the shifted form, which
    loses five of them to overlap, 20 in the unshifted form, which loses four."""
    for name, form in (("512^3 K=3 unshifted, full", "unshifted"),
                       ("512^3 K=3 shifted", "shifted")):
        for c in (cases[name]["head"][0], cases[name]["list"][0]):
            assert (c["nw"], c["ntx"], c["trimmed"], c["nty"]) == (12, 4, 1, 32), name
            assert c["rows"] - LOST[form] == 16, name
    assert cases["512^3 K=3 shifted"]["head"][0]["rows"] == 21


def test_lists_are_sorted_and_free_of_duplicates(cases):
    """Every list is non-empty wherever a footprint fits, in the model's order (a twin
    with a shorter z-chunk right behind its tiling, at the same cost), without duplicates;
    nothing fits: no candidates, no list."""
    empty = 0
    for name, c in cases.items():
        if c["candidates"] == 0:
            assert c["kind"] == "none" and c["head"] == [] and c["list"] == []
            empty += 1
            continue
        assert len(c["list"]) >= 1, name
        costs = [e["cost"] for e in c["list"]]
        assert costs == sorted(costs), name
        head = [e["cost"] for e in c["head"]]
        assert head == sorted(head) and len(head) == min(20, c["candidates"]), name
        keys = [tuple(sorted(e.items())) for e in c["list"]]
        assert len(set(keys)) == len(keys), name
        if c["kind"] in ("single", "seeded", "forced"):
            assert len(c["list"]) == 1, name
        if c["kind"] in ("single", "forced"):
            assert c["list"][0] == c["head"][0], name
    assert empty == 3
    assert cases["128^3 K=3 unshifted"]["kind"] == "single"
    seeded = cases["512^3 K=2 seeded by a settled depth-3 plan"]
    assert seeded["kind"] == "seeded"
    assert (seeded["list"][0]["nw"], seeded["list"][0]["ntx"]) == (12, 1)
    assert cases["512^3 K=2 unseeded"]["kind"] == "full"
    assert cases["512^3 K=3 unshifted, a shifted plan exists: short"]["kind"] == "short"
    # rows that are not whole vectors: 12 waves only
    for name in ("nz=512 ny=512 nx=511 K=3 unshifted", "nz=256 ny=256 nx=510 pitch=512 K=3"):
        assert {e["nw"] for e in cases[name]["head"] + cases[name]["list"]} == {12}, name


def test_trimmed_twins_get_on_a_list_by_rank_only(cases):
    """Per workgroup size a list holds the model's best r tilings and, behind them, the
    tilings with few tiles along x: a trimmed twin is always among the first r."""
    seen = 0
    for name, c in cases.items():
        if c["kind"] not in BEST:
            continue
        tilings = {}
        for e in c["list"]:
            t = tuple(sorted((k, v) for k, v in e.items() if k != "zchunk"))
            mine = tilings.setdefault(e["nw"], [])
            if t not in mine:
                mine.append(t)
        for nw, mine in tilings.items():
            for rank, t in enumerate(mine):
                if dict(t)["trimmed"]:
                    assert rank < BEST[c["kind"]], (name, nw, rank)
                    seen += 1
    assert seen >= 10


# ---- the sampling state machine

class Replay:
    """pdk_plan_check --replay as a child process: one command, one answer."""

    def __init__(self, exe):
        self.p = subprocess.Popen([exe, "--replay"], stdin=subprocess.PIPE,
                                  stdout=subprocess.PIPE, text=True, bufsize=1)

    def tell(self, line):
        self.p.stdin.write(line + "\n")
        self.p.stdin.flush()

    def ask(self, line):
        self.tell(line)
        return self.p.stdout.readline().split()

    def launch(self, plan, sample=1):
        word, cand, how = self.ask("launch %s %d" % (plan, sample))
        assert word == "run"
        return int(cand), how

    def number(self, line):
        return int(self.ask(line)[1])

    def feed(self, plan, times):
        """times[c]: candidate c's samples in the order they come back."""
        for c, ts in enumerate(times):
            for t in ts:
                self.tell("sample %s %d %r" % (plan, c, t))

    def close(self):
        self.p.stdin.close()
        assert self.p.stdout.read() == ""
        assert self.p.wait() == 0


@pytest.fixture
def replay(exe):
    r = Replay(exe)
    yield r
    r.close()


@pytest.fixture(scope="module")
def constants(programs):
    out = subprocess.run([programs["plain"], "--constants"], check=True,
                         stdout=subprocess.PIPE, text=True).stdout.split()
    rounds, final_rounds, band = int(out[0]), int(out[1]), float(out[2])
    assert (rounds, final_rounds) == (2, 6) and abs(band - 1.06) < 1e-6
    return rounds, final_rounds, band


def test_samples_are_issued_round_by_round(replay, constants):
    """Nothing has come back: everybody is owed kFinalRounds, issued in turn; then every
    sample is in flight and the launches run candidate 0, untimed."""
    rounds, final_rounds, _ = constants
    replay.tell("plan p 3")
    assert replay.number("owed p") == 3 * final_rounds
    got = [replay.launch("p") for _ in range(3 * final_rounds)]
    assert got == [(c, "timed") for _ in range(final_rounds) for c in range(3)]
    assert got[:3 * rounds] == [(0, "timed"), (1, "timed"), (2, "timed")] * rounds
    assert replay.number("owed p") == 0
    assert [replay.launch("p") for _ in range(2)] == [(0, "untimed")] * 2


def test_a_runs_first_launch_is_never_timed(replay):
    replay.tell("plan p 3")
    assert replay.launch("p", sample=0) == (0, "untimed")
    assert replay.launch("p") == (0, "timed")
    assert replay.launch("p", sample=0) == (0, "untimed")
    replay.feed("p", [[1.3], [1.1], [1.2]])
    assert replay.launch("p", sample=0) == (1, "untimed")      # the best known so far
    assert replay.launch("p") == (1, "timed")
    assert replay.number("owed p") == 3 * 6 - 2


def test_finalists_are_those_within_the_band(replay, constants):
    """After kRounds samples each, whoever is within kFinalBand of the best is owed
    kFinalRounds; the others stop at kRounds."""
    rounds, final_rounds, band = constants
    replay.tell("plan p 3")
    for _ in range(3 * rounds):
        replay.launch("p")
    replay.feed("p", [[1.0] * rounds, [1.05] * rounds, [1.10] * rounds])
    assert 1.05 < band * 1.0 < 1.10
    more = final_rounds - rounds
    assert replay.number("owed p") == 2 * more
    got = [replay.launch("p") for _ in range(2 * more)]
    assert got == [(0, "timed"), (1, "timed")] * more
    assert replay.launch("p") == (0, "untimed")        # all in flight: the best known
    assert replay.ask("poll p") == ["chosen", "-1"]


def test_nobody_is_dropped_on_one_sample(replay, constants):
    rounds, final_rounds, _ = constants
    replay.tell("plan p 3")
    for _ in range(3):
        replay.launch("p")
    replay.feed("p", [[1.0], [1.0], [5.0]])
    assert [replay.launch("p") for _ in range(3)] == [(0, "timed"), (1, "timed"), (2, "timed")]
    # ... and its second sample decides: 1.0 puts it among the finalists
    replay.feed("p", [[1.0], [1.0], [1.0]])
    assert replay.number("owed p") == 3 * (final_rounds - rounds)


def test_a_lost_sample_is_issued_again(replay):
    replay.tell("plan p 2")
    assert [replay.launch("p") for _ in range(2)] == [(0, "timed"), (1, "timed")]
    replay.tell("lost p 0")
    assert replay.number("owed p") == 2 * 6 - 1
    assert replay.launch("p") == (0, "timed")          # round 1 again
    assert replay.launch("p") == (0, "timed")          # round 2
    assert replay.launch("p") == (1, "timed")


def _settle(replay, times):
    """Explore a plan to the end on a device that answers at once; times[c]: the samples
    of candidate c in order.  Returns what was run and the choice."""
    replay.tell("plan p %d" % len(times))
    left = [list(ts) for ts in times]
    ran = []
    for _ in range(6 * len(times) + 1):
        cand, how = replay.launch("p")
        if how == "settled":
            assert all(not ts for ts in left), left
            return ran, cand
        assert how == "timed"
        ran.append(cand)
        replay.tell("sample p %d %r" % (cand, left[cand].pop(0)))
    raise AssertionError("the plan did not settle")


def test_second_smallest_warm_sample_decides(replay):
    """Candidate 0 has the smallest sample (0.96) and a fast first one (0.95), but is
    otherwise slower than the steady candidate 1: by the minimum, or with the cold first
    sample counted, it would win."""
    ran, chosen = _settle(replay, [[0.95, 0.96, 1.04, 1.04, 1.04, 1.04],
                                   [1.30, 1.00, 1.00, 1.00, 1.00, 1.00]])
    assert chosen == 1 and ran == [0, 1] * 6


@pytest.mark.parametrize("warm,chosen", [(1.05, 0), (1.07, 1)])
def test_fewer_samples_are_scored_best_times_band(replay, warm, chosen):
    """Candidate 1 is outside the band of candidate 0's lucky 0.90 and stops at two
    samples of 1.00: its score is 1.06, against the finalist's second smallest warm one."""
    ran, got = _settle(replay, [[1.2, 0.90] + [warm] * 4, [1.0, 1.0]])
    assert ran == [0, 1, 0, 1, 0, 0, 0, 0]
    assert got == chosen


def test_the_choice_is_for_good(replay):
    _, chosen = _settle(replay, [[1.3, 1.0, 1.0, 1.0, 1.0, 1.0], [1.3] + [1.05] * 5])
    assert chosen == 0
    replay.feed("p", [[9.0] * 3, [0.1] * 6])
    assert replay.ask("poll p") == ["chosen", "0"]
    assert replay.launch("p") == (0, "settled")
    assert replay.launch("p", sample=0) == (0, "settled")


def test_donation_states(replay, constants):
    """What a long run gives up for the unshifted plan: nothing until the shifted plan has
    issued its samples; then what the unshifted plan is owed plus one (a run's first launch
    is no sample) -- for a plan that is not made yet, kFinalRounds per entry of its list;
    -1 once that plan has settled, or would be made settled."""
    _, final_rounds, _ = constants
    replay.tell("plan s 2")
    assert replay.number("donation s - 5") == 0
    for i in range(2 * final_rounds):
        assert replay.number("donation s - 5") == 0
        replay.launch("s")
    assert replay.number("owed s") == 0
    assert replay.number("donation s - 5") == 5 * final_rounds + 1
    assert replay.number("donation s - 1") == -1
    replay.tell("lost s 1")                              # one to take again: not yet
    assert replay.number("donation s - 5") == 0
    replay.launch("s")
    replay.tell("plan u 3")
    assert replay.number("donation s u") == 3 * final_rounds + 1
    for _ in range(6):
        replay.launch("u")
    replay.feed("u", [[1.0, 1.0], [1.0, 1.0], [2.0, 2.0]])
    owed = replay.number("owed u")
    assert owed == 2 * (final_rounds - 2)
    assert replay.number("donation s u") == owed + 1
    for _ in range(owed):
        replay.launch("u")
    assert replay.number("donation s u") == 1            # all in flight: the first launch's
    replay.feed("u", [[1.0] * 4, [1.1] * 4, []])
    assert replay.ask("poll u") == ["chosen", "0"]
    assert replay.number("donation s u") == -1
