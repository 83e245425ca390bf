"""Every entry point of include/s3hip.h that takes an ``s3_stream`` has a case in tests/stream_cases.py, or a stated reason not to
(no GPU needed): a new streamed entry point without a case fails here, before it reaches a GPU."""
import os
import re

import pytest

from tests import stream_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def streamed_entry_points(text=None):
    """the functions of the header whose parameter list has an ``s3_stream`` (comments stripped, as tests/test_abi.py reads it)"""
    if text is None:
        text = open(os.path.join(ROOT, "include", "s3hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    found = {}
    for name, params in re.findall(r"\b(s3_[a-z0-9_]+)\s*\(([^;{]*?)\)\s*;", text, flags=re.S):
        found[name] = bool(re.search(r"\bs3_stream\b", params))
    return sorted(n for n, streamed in found.items() if streamed), sorted(found)


def problems(table, not_cases, streamed, cases):
    """what is wrong with a table: entry points without a case or a reason, names the header does not have, and every difference
    between the table and what the cases themselves say they cover"""
    out = [f"no case: {n}" for n in sorted(set(streamed) - set(table) - set(not_cases))]
    out += [f"not a streamed entry point: {n}" for n in sorted((set(table) | set(not_cases)) - set(streamed))]
    out += [f"both a case and a reason: {n}" for n in sorted(set(table) & set(not_cases))]
    from_cases = {}
    for c in cases.values():
        if not c.covers:
            out.append(f"case {c.name} covers nothing")
        for entry in c.covers:
            from_cases.setdefault(entry, set()).add(c.name)
    for entry in sorted(set(table) | set(from_cases)):
        listed, said = set(table.get(entry, ())), from_cases.get(entry, set())
        out += [f"{entry}: the table lists {n}, the case does not cover it (or does not exist)" for n in sorted(listed - said)]
        out += [f"{entry}: case {n} covers it, the table does not list it" for n in sorted(said - listed)]
        if len(listed) != len(table.get(entry, ())):
            out.append(f"{entry}: a case listed twice")
    return out


def test_parser_sees_the_header():
    streamed, every = streamed_entry_points()
    from tests.test_abi import declared_symbols
    assert every == declared_symbols()                                  # the same functions tests/test_abi.py finds
    assert len(streamed) == 77
    assert "s3_trace" in streamed and "s3_interp_planned_src" in streamed and "s3_mask_mesh" in streamed
    assert "s3_interp_plan_route" not in streamed and "s3_topo_refine" not in streamed and "s3_knn_info" not in streamed


def test_every_streamed_entry_point_has_a_case_or_a_reason():
    """... and the table (entry point -> cases) is the inverse of what the cases say they cover"""
    streamed, _ = streamed_entry_points()
    assert problems(sc.TABLE, sc.NOT_CASES, streamed, sc.CASES) == []


def test_deleting_any_case_name_fails():
    """the check above, turned on itself: it fails without any one name of the table, any one case, any one reason"""
    streamed, _ = streamed_entry_points()
    for entry, names in sc.TABLE.items():
        for name in names:
            table = dict(sc.TABLE)
            table[entry] = tuple(n for n in names if n != name)
            assert problems(table, sc.NOT_CASES, streamed, sc.CASES), (entry, name)
    for name in sc.CASES:
        assert problems(sc.TABLE, sc.NOT_CASES, streamed, {k: v for k, v in sc.CASES.items() if k != name}), name
    for name in sc.NOT_CASES:
        assert problems(sc.TABLE, {k: v for k, v in sc.NOT_CASES.items() if k != name}, streamed, sc.CASES), name


WAITS = ("hipDeviceSynchronize", "hipFree", "DevBuf<")      # a device-wide wait; a scoped device buffer: its release (hipFree) is one


def cited(reason):
    """``csrc/<file>: <function>: "<statement>"`` of a reason -> (the text of the function before the statement, the text after it);
    fails where the file, the function or the statement is not there.  No line numbers: they drift with every edit above them."""
    m = re.search(r'(csrc/[\w./]+): (\w+): "([^"]+)"', reason)
    assert m, f"no citation of the form csrc/<file>: <function>: \"<statement>\" in {reason!r}"
    text = open(os.path.join(ROOT, "sparsespatialsampling_amd", m.group(1))).read()
    start = re.search(r"^(?:extern \"C\" )?(?:static )?int " + m.group(2) + r"\(", text, flags=re.M)
    assert start, f"{m.group(1)} defines no function {m.group(2)}"
    body = text[start.start():text.index("\n}\n", start.start())]
    assert m.group(3) in body, f"{m.group(2)} of {m.group(1)} has no statement {m.group(3)!r}"
    assert any(w in m.group(3) for w in WAITS), f"{m.group(3)!r} is no wait for the whole device"
    return body[:body.index(m.group(3))], body[body.index(m.group(3)):]


def test_not_cases_holds_only_what_it_may():
    """the wait itself, the collectives, and entry points whose cited statement waits for the whole device BEFORE their first launch"""
    for name, reason in sc.NOT_CASES.items():
        assert isinstance(reason, str) and reason.strip(), name
        if name == "s3_stream_synchronize" or name.startswith("s3_comm_"):
            continue
        before, _ = cited(reason)
        assert "<<<" not in before, f"{name}: a kernel is launched before the cited wait: the entry point can have a case"


def test_side_only_cases_cite_the_wait_before_their_main_launch():
    """a case without a control belongs to an entry point that has cases with one, and cites the statement whose release waits for the
    whole device with a launch still to come after it"""
    assert not set(sc.SIDE_ONLY) & set(sc.CASES)
    for c in sc.SIDE_ONLY.values():
        assert c.covers and all(entry in sc.TABLE for entry in c.covers), c.name
        _, after = cited(c.insensitive)
        assert "<<<" in after, f"{c.name}: nothing is launched after the cited wait"


def test_the_citation_check_refuses_a_wrong_one():
    for reason in ('csrc/plan_build.hip: s3_gather_rows: "no such statement;"', 'csrc/plan_build.hip: s3_no_such_function: "s3::DevBuf<int32_t> d_bad;"',
                   "csrc/plan_build.hip:471: a line number", 'csrc/plan_build.hip: s3_gather_rows: "S3_LAUNCH_CHECK();"'):
        with pytest.raises(AssertionError):
            cited(reason)


def test_a_new_entry_point_without_a_case_is_caught():
    text = open(os.path.join(ROOT, "include", "s3hip.h")).read()
    text = text.replace("int s3_stream_synchronize(s3_stream stream);",
                        "int s3_stream_synchronize(s3_stream stream);\nint s3_new_kernel(const double *d_x, int64_t n,\n    s3_stream stream);")
    streamed, _ = streamed_entry_points(text)
    assert problems(sc.TABLE, sc.NOT_CASES, streamed, sc.CASES) == ["no case: s3_new_kernel"]


def test_cases_state_the_poison_rule():
    assert "VALID input" in sc.__doc__ and sc.DELAY_FACTOR == 4
    with pytest.raises(AssertionError):
        sc.case("idw_weights", "s3_idw_weights")(lambda: None)          # a second case of one name
