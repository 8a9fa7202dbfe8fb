"""CPU: tests/domain.py against csrc/*.hip, against tests/test_gpu_domain.py's case lists, and against itself.

  * every top-level `&&` conjunct of the in-scope entries' RECALGO_REQUIRE lines has a row, every row a conjunct: a check
    that is added, changed or removed without its row fails here - and so a refusal case can only exist for a check the
    source really makes;
  * every `at` / `outside` tag is a case tests/test_gpu_domain.py parametrises, and every case belongs to a row;
  * an at-limit case is a valid call ON the boundary: every conjunct holds, and no valid call lies between it and the first
    value that fails its row;
  * a refusal case is a valid call in which exactly the row's quantity is changed, and then exactly the row (and what it
    implies, `also`) fails;
  * the arguments the table evaluates are the header's, in the header's order.
Three planted faults show that each of the first, second and fourth is reported.
"""
import os
import re

import pytest

from tests import domain as D
from tests import test_gpu_domain as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "recalgorithm_amd", "csrc")


def _source(unit):
    with open(os.path.join(CSRC, unit)) as f:
        return f.read()


SOURCES = {unit: _source(unit) for unit in D.UNITS}
UNIT_OF = {"recalgo_" + n: unit for unit, names in D.UNITS.items() for n in names}


# ---- the checks, as functions that return what is wrong (the planted faults call them too) ------------------------------------
def table_vs_source(entry, src, table=D.DOMAIN):
    got, want = D.source_conjuncts(src, entry), list(table[entry])
    problems = [f"{entry}: `{c}` is checked by the source and has no row" for c in got if c not in want]
    problems += [f"{entry}: the row `{c}` names no check of the source" for c in want if c not in got]
    problems += [f"{entry}: `{c}` is checked twice" for c in set(got) if got.count(c) > 1]
    return problems


def rows_vs_cases(entry, table=D.DOMAIN, at_cases=G.AT_CASES, outside_cases=G.OUTSIDE_CASES):
    problems = []
    used_at, used_out = set(), set()
    for row in table[entry].values():
        if bool(row.at) == bool(row.not_driven) and row.kind != "pointer":
            problems.append(f"{entry} `{row.text}`: an at-limit case or a not_driven reason, one of the two")
        if row.not_driven and row.not_driven != D.BIG:
            problems.append(f"{entry} `{row.text}`: not_driven for another reason than size")
        if not row.outside:
            problems.append(f"{entry} `{row.text}`: no refusal case")
        for tag, cases, used in [(t, at_cases, used_at) for t in row.at] + [(t, outside_cases, used_out) for t in row.outside]:
            if cases.get(D.case_id(entry, tag)) != (entry, tag):
                problems.append(f"{entry} `{row.text}`: tests/test_gpu_domain.py has no case {D.case_id(entry, tag)}")
            used.add(tag)
    for cases, used, what in ((at_cases, used_at, "at-limit"), (outside_cases, used_out, "refusal")):
        problems += [f"the {what} case {cid} belongs to no row" for cid, (e, t) in cases.items() if e == entry and t not in used]
    return problems


def outside_case_is_one_step(entry, row, tag):
    neighbour, change = D.outside_dims(entry, row, tag)
    problems = [f"{entry} {tag}: the neighbour fails `{c}`" for c, ok in D.evaluate(entry, neighbour).items() if not ok]
    before, after = D.full(entry, neighbour), D.full(entry, neighbour, change)
    args = [n for n, _ in D.ENTRIES[entry]["args"]]
    moved = sorted(n for n in args if before[n] != after[n])
    if len(moved) != 1 or moved[0] not in row.quantity.split("|"):
        problems.append(f"{entry} {tag}: differs from its valid neighbour in {moved}, the row names {row.quantity}")
    failing = {c for c, ok in D.evaluate(entry, neighbour, change).items() if not ok}
    if failing != {row.text} | set(row.also):
        problems.append(f"{entry} {tag}: fails {sorted(failing)}, not exactly `{row.text}`")
    return problems


def at_case_is_on_the_boundary(entry, row, tag):
    dims = D.at_dims(entry, tag)
    if dims.get("B") == 0 or dims.get("M") == 0:       # the entry returns before its later checks: only the row itself
        return [] if D.evaluate(entry, dims, rows=[row.text])[row.text] else [f"{entry} {tag}: fails its own row"]
    problems = [f"{entry} {tag}: fails `{c}`" for c, ok in D.evaluate(entry, dims).items() if not ok]
    if row.kind not in ("limit", "lds") or problems:
        return problems
    # walk the quantity towards the outside: every value before the first that fails the row must be no valid call
    names = [n for n in row.quantity.split("|") if n in D.parse_tag(tag)] or row.quantity.split("|")[:1]
    q = names[0]
    for step in (1, -1):
        for k in range(1, 9):
            moved = {**dims, q: D.full(entry, dims)[q] + step * k}
            holds = D.evaluate(entry, moved)
            if not holds[row.text]:
                return problems
            if all(holds.values()):
                break                                   # a valid call farther out in this direction: not the boundary
    return problems + [f"{entry} {tag}: {q} = {dims.get(q)} is not the last value `{row.text}` accepts"]


# ---- the table ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry", list(D.ENTRIES))
def test_every_check_has_its_row_and_every_row_its_check(entry):
    assert table_vs_source(entry, SOURCES[UNIT_OF[entry]]) == []
    assert all(r.kind in D.KINDS for r in D.DOMAIN[entry].values())


@pytest.mark.parametrize("entry", list(D.ENTRIES))
def test_every_row_has_its_cases_and_every_case_its_row(entry):
    assert rows_vs_cases(entry) == []
    tags = [t for r in D.DOMAIN[entry].values() for t in r.outside]
    assert len(tags) == len(set(tags)), "one refusal case, one row"


def test_case_lists_cover_exactly_the_table():
    assert {e for e, _ in G.AT_CASES.values()} | {e for e, _ in G.OUTSIDE_CASES.values()} == set(D.ENTRIES)
    assert all(callable(G._driver(e)) for e in D.ENTRIES)


@pytest.mark.parametrize("entry", list(D.ENTRIES))
def test_at_limit_cases_are_valid_calls_on_the_boundary(entry):
    assert [p for r in D.DOMAIN[entry].values() for t in r.at for p in at_case_is_on_the_boundary(entry, r, t)] == []


@pytest.mark.parametrize("entry", list(D.ENTRIES))
def test_refusal_cases_change_one_quantity_and_fail_one_row(entry):
    assert [p for r in D.DOMAIN[entry].values() for t in r.outside for p in outside_case_is_one_step(entry, r, t)] == []


def test_arguments_are_the_headers():
    with open(os.path.join(ROOT, "include", "recalgo.h")) as f:
        header = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    for entry, e in D.ENTRIES.items():
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % entry, header)
        assert m, entry
        names = [re.search(r"(\w+)\s*$", p).group(1) for p in m.group(1).split(",")]
        assert names == [n for n, _ in e["args"]] + ["stream"], entry
        assert names == D._definition(SOURCES[UNIT_OF[entry]], entry)[0], f"{entry}: the definition's parameters"
        for (n, how), p in zip(e["args"], m.group(1).split(",")):
            assert ("*" in p) == (how != "int"), f"{entry}: {n}"


def test_kinds_are_counted():
    counts = {k: sum(r.kind == k for rows in D.DOMAIN.values() for r in rows.values()) for k in D.KINDS}
    assert sum(counts.values()) == sum(len(rows) for rows in D.DOMAIN.values()) and all(counts.values())


# ---- planted faults -----------------------------------------------------------------------------------------------------
def test_planted_a_removed_check_is_reported():
    src = SOURCES["cross.hip"]
    assert "d <= 1024 && L >= 1" in src
    planted = src.replace("d <= 1024 && L >= 1", "L >= 1")
    got = table_vs_source("recalgo_cross_fwd", planted)
    assert got == ["recalgo_cross_fwd: the row `d <= 1024` names no check of the source"]
    widened = src.replace("d <= 1024 && L >= 1", "d <= 2048 && L >= 1")
    assert len(table_vs_source("recalgo_cross_bwd", widened)) == 2            # the new check has no row, the old row no check
    # a forwarding entry is held to the entry it forwards to
    assert table_vs_source("recalgo_embedding_gather_fwd", SOURCES["embed.hip"].replace("F > 0 && K > 0 && out_stride", "K > 0 && out_stride")) \
        == ["recalgo_embedding_gather_fwd: the row `F > 0` names no check of the source"]


def test_planted_a_row_without_a_case_is_reported():
    entry = "recalgo_attention_pool_bwd"
    at = {k: v for k, v in G.AT_CASES.items() if k != "attention_pool_bwd-P4096"}
    got = rows_vs_cases(entry, at_cases=at)
    assert got == ["recalgo_attention_pool_bwd `smem <= kLdsDefault`: tests/test_gpu_domain.py has no case attention_pool_bwd-P4096"]
    rows = dict(D.DOMAIN[entry])
    rows["P <= 4096"] = D.Row("P <= 4096", "limit", "P", (), ("P4097",), (), None)
    assert any("an at-limit case or a not_driven reason" in p for p in rows_vs_cases(entry, table={entry: rows}))
    orphan = dict(G.OUTSIDE_CASES, **{"attention_pool_bwd-K66": (entry, "K66")})
    assert rows_vs_cases(entry, outside_cases=orphan) == ["the refusal case attention_pool_bwd-K66 belongs to no row"]


def test_planted_an_outside_case_that_changes_two_quantities_is_reported():
    entry = "recalgo_cross_fwd"
    row = D.DOMAIN[entry]["d <= 1024"]
    assert outside_case_is_one_step(entry, row, row.outside[0]) == []
    # d = 1028 next to the smallest call: x_stride and out_stride (8) are too short as well
    got = outside_case_is_one_step(entry, row, "d1028")
    assert len(got) == 1 and "not exactly `d <= 1024`" in got[0] and "x_stride >= d" in got[0]
    # two arguments moved at once
    two = D.Row(row.text, "limit", "d|L", row.at, ("x_stride1028,out_stride1028,d1028,L7",), (), None)
    got = outside_case_is_one_step(entry, two, two.outside[0])
    assert any("differs from its valid neighbour in ['L', 'd']" in p for p in got)
    # and an at-limit case one short of the boundary
    short = D.DOMAIN["recalgo_attention_pool_bwd"]["smem <= kLdsDefault"]
    assert at_case_is_on_the_boundary("recalgo_attention_pool_bwd", short, "P4095") \
        == ["recalgo_attention_pool_bwd P4095: P = 4095 is not the last value `smem <= kLdsDefault` accepts"]
