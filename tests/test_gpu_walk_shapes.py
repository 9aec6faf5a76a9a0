"""The walk (csrc/bfs_device.h k_bfs, bfs_narrow, replay_slow, bfs_chunk_wide, the visited index) on the designed inputs of
tests/walk_shapes.py (tests/test_walk_shapes_model.py checks without a GPU that every input has the shape named here), against the
oracle's walk (oracle/pyoracle.py bfs) in order, distances, coverages, `last` flags and levels, with no tolerance:

  case                  what its widths make the kernel do
  fan-256               1, 4, 16, 64, 256 ... 256, 64, 16, 4, 1: levels of two and four chunks; the four parents of a merged vertex half
                        in one chunk (lds_set_min, the smallest rank wins), half in a later one (vis_find sees the earlier chunk's)
  fan-128 / fan-129     a level of exactly 512 candidates, and of 516 (4 neighbours); fan-64 / fan-65: 512 and 520 (8 neighbours)
  fan-16 / fan-17       a frontier of flim and of flim + 1 vertices with 4 neighbours; fan-8 / fan-9 with 8 (and, with 4, the scouts' limit)
  fan-256-weak          three copies a read, three words with two: coverage at the threshold and one under it
  ragged                six walkers that end one at a time: inside a predicted stretch, 64 levels behind the fan-out, a level later
  branch-p              one walker becomes two at level p + 1: p = 20, 64, 65, 128, 129
  cycle-150, cycle-k+9  the path returns to the seed: the visited index ends the walk inside a predicted stretch
  seeds-*               duplicates inside a seed chunk, 700 windows and a chunk apart, inside a narrow level 0; 512 and 513 windows; a
                        first chunk with nothing solid
  collide-n[-wide]      n k-mers with the fingerprint and the home bucket of a vertex in front of it in the visited index

All cases of one (k, key mode) are counted into one table (their seeds are random: their graphs are apart; the oracle walks the same
table).  Limits come from the oracle's unbounded walk: --maxkmers at the first and the last vertex a chunk accepts and to either side,
the radius at a wide level and beside it, the cap between the walkers of a narrow level.  Forms: the default (a companion scouts),
MC_BFS_COMPANION=0 (the verifier scouts itself), MC_BFS_DIRECT=0 (a copy of the solid k-mers), MC_BFS_SELFCHECK=1 (the device-side
check must agree), and a batch of 65 jobs (no companion beyond 64).  MC_BFS_STATS' line says where a walk went: chunks_wide is
ceil(seed windows / 512) + the sum of ceil(W nb / 512) over the levels wider than flim, as k_bfs counts."""
import functools
import re

import numpy as np
import pytest

from oracle import pyoracle as po
from tests import walk_shapes as ws
from tests.helpers import assert_bfs_equal, seed_windows

gpu = pytest.mark.gpu

FORMS = {"default": {}, "inline": {"MC_BFS_COMPANION": "0"}, "solid": {"MC_BFS_DIRECT": "0"}, "selfcheck": {"MC_BFS_SELFCHECK": "1"}}
SWITCHES = ("MC_COUNT_PATH", "MC_LONG_RECORDS", "MC_LONG_BINS", "MC_SUPERKMERS", "MC_BFS_DIRECT", "MC_BFS_COMPANION", "MC_BFS_SELFCHECK",
            "MC_BFS_TRACE_DUMP")
FAN_KEYS = [(21, po.KEY_PACKED), (31, po.KEY_PACKED), (32, po.KEY_POLY), (63, po.KEY_POLY)]
OTHER_KEYS = [(31, po.KEY_PACKED), (41, po.KEY_POLY)]
COLLIDE_KEYS = [(32, po.KEY_POLY), (32, po.KEY_FNV1A), (40, po.KEY_POLY), (63, po.KEY_POLY)]
FAR = 10000   # a radius no case reaches: mc_bfs wants one limit set
STATS = re.compile(r"\[bfs job (\d+)\] n=(\d+) level=(-?\d+) rounds_narrow=(\d+) \(slow (\d+)\) chunks_wide=(\d+) scout calls=(\d+) hops=(\d+) ")
FAN_NAMES = ["fan-%d" % m for _, m, _, _ in ws.FAN_TABLE]
OTHER_NAMES = ["fan-256-weak", "ragged"] + ["branch-%d" % p for p in ws.BRANCH_P] + ["cycle-150", "cycle-k+9"] + ["seeds-" + s for s in ws.SEED_KINDS]
COLLIDE_NAMES = ["collide-%d%s" % (n, w) for n in (1, 2, 3) for w in ("", "-wide")]


@pytest.fixture(scope="module")
def mc():
    import metacherchant_amd as m
    m.native.load()
    yield m
    for ctx in _contexts.values():
        ctx.close()
    _contexts.clear()


@functools.lru_cache(maxsize=None)
def cases(k, mode):
    out = {}
    if (k, mode) in FAN_KEYS:
        out.update((c.name, c) for c in ws.fans(k))
    if (k, mode) in OTHER_KEYS:
        out.update(("cycle-k+9" if c.name == "cycle-%d" % (k + 9) else c.name, c) for c in ws.others(k))
    if (k, mode) in COLLIDE_KEYS:
        out.update((c.name, c) for c in ws.collisions(k))
    return out


@functools.lru_cache(maxsize=None)
def store(k, mode):
    reads = [r for c in cases(k, mode).values() for r in c.reads]
    off = np.zeros(len(reads) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(r) for r in reads])
    return np.concatenate(reads).astype(np.uint8), off


@functools.lru_cache(maxsize=None)
def oracle_table(k, mode):
    t = po.Table()
    t.count_reads(*store(k, mode), k, mode)
    return t


_contexts = {}
_report = []   # the figures of a test's walks (capfd is emptied before every walk): printed behind the test, python -m pytest -rP


@pytest.fixture(autouse=True)
def report():
    _report.clear()
    yield
    print("\n".join(_report))


def context(mc, k, mode, form):
    """one context a (k, key mode, form), with every case of that key counted; the switches are read by mc_create"""
    if (k, mode, form) not in _contexts:
        with pytest.MonkeyPatch.context() as mp:
            for n in SWITCHES:
                mp.delenv(n, raising=False)
            mp.setenv("MC_BFS_STATS", "1")
            for n, v in FORMS[form].items():
                mp.setenv(n, v)
            ctx = mc.Context(k, mode, 0, 0)
        codes, off = store(k, mode)
        ctx.add_reads_packed(po.pack(codes), off)
        assert ctx.finalize() == oracle_table(k, mode).size()
        _contexts[(k, mode, form)] = ctx
    return _contexts[(k, mode, form)]


@functools.lru_cache(maxsize=None)
def windows(k, mode, name, direction):
    his, los = zip(*[seed_windows(s, k) for s in cases(k, mode)[name].seeds_for(direction)])
    return np.concatenate(his), np.concatenate(los)


@functools.lru_cache(maxsize=None)
def want(k, mode, name, direction, min_cov, mk, mr):
    return po.bfs(oracle_table(k, mode), k, mode, cases(k, mode)[name].seeds_for(direction), direction, min_cov, mk, mr)


def stats_of(capfd):
    """job -> (rounds_narrow, slow, chunks_wide, hops) of the walks since the last call"""
    return {int(m[0]): tuple(int(x) for x in (m[3], m[4], m[5], m[7])) for m in STATS.findall(capfd.readouterr().err)}


def check_path(name, k, mode, direction, w, st, label):
    """the walk went where its widths send it"""
    c = cases(k, mode)[name]
    rounds, slow, chunks, hops = st
    widths = ws.histogram(w)
    formula = ws.chunks_expected(c.n_seed_windows, widths, direction)
    _report.append("walk shapes: %s k=%d mode=%d dir=%d %s: n=%d chunks_wide %d formula %d rounds_narrow %d slow %d hops %d" % (
        name, k, mode, direction, label, len(w["lo"]), chunks, formula, rounds, slow, hops))
    assert chunks == formula, (name, direction, label, chunks, formula)
    assert (rounds > 0) == any(0 < x <= ws.flim_of(direction) for x in widths), (name, direction, label, rounds)
    return rounds, slow, chunks, hops


def one_walk(mc, capfd, k, mode, form, name, direction, mk, mr, min_cov=None):
    c = cases(k, mode)[name]
    min_cov = c.min_cov if min_cov is None else min_cov
    ctx = context(mc, k, mode, form)
    hi, lo = windows(k, mode, name, direction)
    capfd.readouterr()
    got = ctx.bfs(hi if k > 32 else None, lo, direction, min_cov, mk, mr)
    w = want(k, mode, name, direction, min_cov, mk, mr)
    assert w is not None
    assert_bfs_equal(got, w)
    return w, check_path(name, k, mode, direction, w, stats_of(capfd)[0], "mk=%d mr=%d" % (mk, mr))


def limits(k, direction, w, level=None):
    """(max_kmers, max_radius) around the expansion of `level`.  Not given: the second level behind level 0 that is wider than flim
    and has a level behind it (the fans' plateau), the only one where there is one, level 0 where nothing else is wide.  Without a
    wide level: the cap between the walkers of the widest narrow level, j levels into it"""
    widths = ws.histogram(w)
    n = len(w["lo"])
    flim = ws.flim_of(direction)
    if level is None:
        wide = [L for L, x in enumerate(widths) if x > flim and 1 <= L < len(widths) - 1]
        level = wide[1] if len(wide) > 1 else wide[0] if wide else 0 if widths[0] > flim else None
    if level is not None:
        n_l = sum(widths[:level + 1])                          # the oracle's n at the start of the level's expansion
        a = ws.first_chunk_accepts(w, k, direction, level)     # what its first chunk accepts
        mks = sorted({x for x in (n_l, n_l + 1, n_l + a - 1, n_l + a, n_l + a + 1, n, n - 1, n + 1) if x >= 1})
        return [(x, -1) for x in mks] + [(-1, r) for r in (level - 1, level, level + 1) if r >= 0] + [(n_l + a, level + 1), (n_l + a + 1, level)]
    F = max(widths)
    at = widths.index(F)
    run = next((i for i, x in enumerate(widths[at:]) if x != F), len(widths) - at)
    j = min(10, max(run - 2, 0))
    n0 = sum(widths[:at + 1])
    return [(n0 + F * j + r, -1) for r in range(F)] + [(n, -1), (n - 1, -1), (-1, at + j), (n0 + F * j + 1, at + j + 1)]


def directions_of(name):
    if name in FAN_NAMES:
        dirs = ws.fan_directions(int(name[4:]))
        return dirs + ((-1,) if 1 in dirs else ())
    return (1,) if name.startswith("collide") else (1, -1, 0)


def run_case(mc, capfd, k, mode, form, name):
    c = cases(k, mode)[name]
    for direction in directions_of(name):
        w, (rounds, slow, chunks, hops) = one_walk(mc, capfd, k, mode, form, name, direction, -1, FAR)
        assert ws.histogram(w) == c.widths(direction), (name, direction)   # (the shape, on the table of all cases)
        if direction == 0 or name.startswith(("branch", "cycle")) or name == "seeds-dup_narrow":
            assert slow > 0, (name, direction, slow)
        if form == "inline" and name.startswith("branch") and direction != 0 and k >= 23:
            assert hops > 0, (name, direction, hops)   # the verifier's own scouts ran
        lims = limits(k, direction, w)
        if name == "fan-256":  # the level whose expansion merges four parents into one vertex, too
            lims += limits(k, direction, w, k)
        if form in ("solid", "selfcheck"):
            lims = lims[1:6:2] + lims[-2:]
        for mk, mr in lims:
            one_walk(mc, capfd, k, mode, form, name, direction, mk, mr)


@gpu
@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("name", FAN_NAMES)
@pytest.mark.parametrize("k,mode", FAN_KEYS)
def test_fans(mc, capfd, k, mode, name, form):
    run_case(mc, capfd, k, mode, form, name)


@gpu
@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("name", OTHER_NAMES)
@pytest.mark.parametrize("k,mode", OTHER_KEYS)
def test_other_shapes(mc, capfd, k, mode, name, form):
    run_case(mc, capfd, k, mode, form, name)


@gpu
@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("k,mode", COLLIDE_KEYS)
def test_collisions_in_the_visited_index(mc, capfd, k, mode, form):
    """a vertex whose fingerprint and home bucket other k-mers of the index have is still found new: through vis_contains from a
    narrow level 0, through vis_find from a wide one; one entry in front of it, a full bucket, a bucket and the next"""
    for name in COLLIDE_NAMES:
        c = cases(k, mode)[name]
        w, _ = one_walk(mc, capfd, k, mode, form, name, 1, -1, FAR)
        assert ws.kmers_of(w)[-1] == c.facts["v2"] and w["dist"][-1] == 1
        one_walk(mc, capfd, k, mode, form, name, 1, len(w["lo"]), -1)
        one_walk(mc, capfd, k, mode, form, name, 1, len(w["lo"]) - 1, -1)


@gpu
@pytest.mark.parametrize("k,mode", OTHER_KEYS)
def test_batch_of_65_jobs(mc, capfd, k, mode):
    """more than 64 jobs a launch: no companion, every verifier scouts for itself (the CLI's batches of one job a seed sequence).
    One threshold a batch: 1, at which every case keeps its shape but the weak fan, which is the full fan there."""
    names = list(cases(k, mode))
    jobs = [(n, d) for d in (1, 0, -1) for n in names]
    jobs = (jobs + jobs)[:65]
    assert len(jobs) == 65 and len({n for n, _ in jobs}) == len(names)
    ctx = context(mc, k, mode, "default")
    capfd.readouterr()
    got = ctx.bfs_batch([(windows(k, mode, n, d)[0] if k > 32 else None, windows(k, mode, n, d)[1], d) for n, d in jobs], 1, 30000, FAR)
    st = stats_of(capfd)
    assert len(got) == len(st) == 65
    for j, (n, d) in enumerate(jobs):
        w = want(k, mode, n, d, 1, 30000, FAR)
        assert w is not None
        assert_bfs_equal(got[j], w)
        rounds, slow, chunks, hops = check_path(n, k, mode, d, w, st[j], "job %d of 65" % j)
        if n.startswith("branch") and d != 0:
            assert hops > 0, (n, d, hops)
