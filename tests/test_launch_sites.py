"""Every kernel launch of the output families sizes its grid through the path that ESIM_GRID_CAP clamps (grid_capped / grid_clamp,
esim_host_ctx.h), or stands on the list below of launches that cover their items exactly, with the reason.  A launch added later
cannot escape the cap unnoticed: tests/test_grid_trips_gpu.py then runs it with one and three workgroups against its reference.
A check of the host code's own text; no GPU needed."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "epidemicsimulator_amd", "csrc")
FILES = ["esim_host_%s.h" % k for k in ("outputs", "settings", "tree", "household", "places", "contacts", "flows", "events", "curves", "compare", "ensrows",
                                        "snapshot", "upload")] + ["esim_curves.h", "esim_pairs.h"]
CLAMPED = re.compile(r"\bgrid_(capped|clamp)\(")

# (file, kernel) -> why its grid is not clamped.  Only launches whose grid covers the items exactly: the kernel has no loop over
# its items, or is told its stretch and must find the workgroups that go with it.
EXACT_COVER = {
    ("esim_host_outputs.h", "k_area_census"): "grid = ceil(n / per_block) with the per_block the kernel is given: a workgroup counts its own stretch in its LDS window of areas",
    ("esim_host_outputs.h", "k_group_finish"): "a lane per group, no loop (grid_for without a cap)",
    ("esim_host_outputs.h", "k_area_vax_replay"): "a workgroup per step of the programme's replay, at most 1024 steps a launch: the host loops over the stretches",
    ("esim_host_outputs.h", "k_series_prefix"): "a lane per column, no loop (grid_for without a cap)",
    ("esim_host_outputs.h", "k_ensemble_fold_arrival"): "a lane per area or group, no loop (grid_for without a cap)",
    ("esim_host_outputs.h", "k_ensemble_fold"): "a lane per area or group, no loop (grid_for without a cap)",
    ("esim_host_tree.h", "k_chain_roots"): "a lane per index case, no loop (grid_for without a cap)",
    ("esim_host_compare.h", "k_compare_prefix"): "a lane per column, no loop (grid_for without a cap)",
    ("esim_host_compare.h", "k_compare_count"): "grid = ceil(n / per_block) with the per_block the kernel is given, as k_area_census",
    ("esim_host_upload.h", "k_restart_books"): "a lane per histogram slot or seed, no loop (grid_for without a cap)",
    ("esim_curves.h", "k_curve_tile"): "a workgroup per tile of the scan",
    ("esim_curves.h", "k_curve_carry"): "one wavefront over the tile aggregates",
    ("esim_curves.h", "k_curve_scan"): "a workgroup per tile of the scan",
    ("esim_pairs.h", "k_pairs_sort_tile"): "a workgroup per tile of the bitonic sort",
    ("esim_pairs.h", "k_pairs_sort_step"): "a lane per compared pair of one step of the bitonic sort",
}
# The stand-alone header takes its bound from the caller: (file, kernel) -> (the bound in the grid, the host file whose call passes the clamped grid, the call).
BOUNDED_BY_CALLER = {("esim_curves.h", "k_curve_reduce"): ("max_blocks", "esim_host_curves.h", "curve_reduce_enqueue(")}


def call_args(text, at):
    """The top-level arguments of the call whose opening parenthesis is text[at]."""
    depth, args, start = 0, [], at + 1
    for i in range(at, len(text)):
        ch = text[i]
        if ch in "([{":
            depth += 1
        elif ch in ")]}":
            depth -= 1
            if depth == 0:
                args.append(text[start:i].strip())
                return args
        elif ch == "," and depth == 1:
            args.append(text[start:i].strip())
            start = i + 1
    raise AssertionError("unbalanced call at offset %d" % at)


def launches(name):
    """(kernel, grid expression, the text before the launch) of every hipLaunchKernelGGL of a file."""
    text = open(os.path.join(CSRC, name)).read()
    for m in re.finditer(r"hipLaunchKernelGGL\(", text):
        args = call_args(text, m.end() - 1)
        kernel = re.match(r"\(?\s*(\w+)", args[0]).group(1)
        yield kernel, args[1], text[:m.start()]


def is_clamped(grid, before):
    if CLAMPED.search(grid):
        return True
    m = re.fullmatch(r"(?:dim3\()?\s*(\w+)\s*\)?", grid)                # a variable: its nearest definition above sizes it
    if not m:
        return False
    defs = list(re.finditer(r"\bconst (?:dim3|uint32_t) %s\b[^;]*;" % re.escape(m.group(1)), before))
    return bool(defs) and bool(CLAMPED.search(defs[-1].group(0)))


def test_every_output_launch_is_clamped_or_covers_its_items_exactly():
    seen, used, n = [], set(), 0
    for name in FILES:
        for kernel, grid, before in launches(name):
            n += 1
            key = (name, kernel)
            if key in BOUNDED_BY_CALLER:
                bound, host, call = BOUNDED_BY_CALLER[key]
                assert bound in grid, (key, grid)
                text = open(os.path.join(CSRC, host)).read()
                at = text.index(call)
                assert CLAMPED.search(call_args(text, at + len(call) - 1)[-1]), "%s: the call in %s does not pass a clamped grid" % (kernel, host)
                used.add(key)
            elif is_clamped(grid, before):
                assert key not in EXACT_COVER, "%s in %s is clamped and on the list of exact covers" % (kernel, name)
            elif key in EXACT_COVER:
                assert EXACT_COVER[key]
                used.add(key)
            else:
                seen.append("%s: %s with grid `%s`" % (name, kernel, grid))
    assert n >= 80
    assert not seen, "launches that neither go through grid_capped / grid_clamp nor are listed as exact covers:\n" + "\n".join(seen)
    stale = sorted((set(EXACT_COVER) | set(BOUNDED_BY_CALLER)) - used)
    assert not stale, "listed launches that no longer exist: %s" % stale


def test_the_state_of_the_ensemble_accumulators_launches_nothing():
    # esim_host_ensemble.h holds the kinds' table, begin, read-out and fold dispatch; every fold's launches stay in its family's file
    text = open(os.path.join(CSRC, "esim_host_ensemble.h")).read()
    assert "hipLaunchKernelGGL" not in text and not CLAMPED.search(text) and "<<<" not in text and "_enqueue(" not in text


def test_the_cap_is_off_unless_the_environment_sets_it_and_is_documented():
    ctx = open(os.path.join(CSRC, "esim_host_ctx.h")).read()
    # by construction: with the knob at 0 the clamp returns the grid it was given before it touches anything
    body = ctx[ctx.index("uint32_t grid_clamp("):]
    assert re.search(r"const uint32_t knob = c->tune\.grid_cap;\s*if \(!knob\) return grid;", body[:body.index("LaunchLog &l")])
    assert "uint32_t grid_cap = 0;" in ctx
    upload = open(os.path.join(CSRC, "esim_host_upload.h")).read()
    assert 'std::getenv("ESIM_GRID_CAP")' in upload and "std::max(1, std::atoi(e))" in upload[upload.index('std::getenv("ESIM_GRID_CAP")'):][:120]
    for doc in ("README.md", "DESIGN.md"):
        assert "ESIM_GRID_CAP" in open(os.path.join(ROOT, doc)).read(), doc
    assert "ESIM_GRID_CAP" not in open(os.path.join(ROOT, "bench.py")).read()
