"""The CPU half of the table-edge sweep (tests/table_edge_cases.py, tests/test_gpu_table_edges.py): the generators put what they claim
where they claim, the restated lengths are the ones the cases are built for, the restated list loads of the capacity designs sit on
the capacity, every sample kind occurs -- and for every planted served cell the host definition of its value (oracle.dtab /
dtab_tail / dtab_combine) lies within 1e-10 relative of the checker's LIBM flavour, i.e. the definition and the reference stay inside
the north-star bar before the device is asked."""
import numpy as np
import pytest

import table_edge_cases as tc

REL_TOL = 1e-10
_CACHE = {}


def cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def multi_cases(oracle):
    return [cached("A", lambda: tc.case_A(oracle)), cached("B", lambda: tc.case_B(oracle))]


def big_cases(oracle):
    return multi_cases(oracle) + [cached("C0", lambda: tc.case_C(oracle, 0)), cached("C1", lambda: tc.case_C(oracle, 1)),
                                  cached("D", lambda: tc.case_D(oracle))]


def test_windows_restated():
    assert tc.tab_windows(304, 7824) == (304, 2920, 2920)
    assert tc.tab_windows(4096, 32768) == (1024, 2560, 2560)
    assert tc.tab_windows(64, 64) == (64, 64, 128)
    assert tc.tab_windows(1024, 2560) == (1024, 2560, 2560)
    assert tc.tab_windows(1032, 2552) == (1024, 2552, 2568)


def test_statistics_read_every_sixteenth_piece():
    assert tc.stat_exons(4095).size == 4095 and tc.stat_exons(130).size == 130
    e = tc.stat_exons(4300)
    assert e.size == 5 * 64 and set(e // 1024) == {0, 1, 2, 3, 4} and (e % 1024 < 64).all()
    assert tc.stat_exons(4096 + 10)[-1] == 4105 and tc.stat_exons(4096 + 10).size == 4 * 64 + 10


def test_grid_restated():
    """edplan::sm_grid, the chunks and the lists, against figures worked out by hand from ed_launch_plan.hpp / k_emit_tab_sm"""
    g = tc.SmGeometry(np.concatenate([[0], np.cumsum(tc.SIZES_4300)]), 130)
    assert g.order[:3] == [0, 8, 9] and g.order[-1] == 2 and 3 not in g.order
    assert g.blocks[0] == (0, 64, 0) and g.blocks[23] == (1472, 1500, 0)          # chromosome 0: 24 blocks, the last one partial
    assert g.blocks[24] == (1949, 1984, 8)                                          # blocks sit on the absolute grid, clipped
    assert g.nsplit == 2 and g.per == (g.nblk + 1) // 2
    assert tc.SmGeometry(np.concatenate([[0], np.cumsum(tc.SIZES_4300)]), 1).nsplit == 2
    assert tc.SmGeometry(np.concatenate([[0], np.cumsum(tc.SIZES_4300)]), 257).nsplit == 2
    c = tc.SmGeometry(np.concatenate([[0], np.cumsum(tc.SIZES_33K)]), 3)
    assert c.nblk >= 512 and c.nsplit == 16
    assert tc.SmGeometry([0, 130], 9).nsplit == 1
    # sample 10 (second round of eight), chunk 1 of 2, wave 3: workgroup ((10 / 8) * 2 + 1) * 8 + 2 = 26 -> list 26 * 16 + 3
    b = g.per + 3 + 16
    assert g.chunk[b] == 1 and g.wave[b] == 3 and g.workgroup(10, 1) == 26 and g.list_of(10, b) == 419
    assert tc.cold_cap_per(4300, 130) == 64 and tc.cold_cap_per(4300, 257) == 67 and tc.cold_cap_per(33100, 1) == 64


def test_plants_leave_the_statistics_alone(oracle):
    """with E >= 4096 no plant sits in an exon the statistics read: the dims restated from the planted matrix are the ones the plants were derived
    from, in both table modes and in the 16-bit variant"""
    for case in big_cases(oracle):
        assert not case["planted"][tc.stat_exons(case["E"])].any()
        for tails in (0, 1):
            for t, r in ((case["test"], case["ref"]), (case["test16"], case["ref16"])):
                dims, wins, _ = tc.restate(oracle, t, r, case["phi"], case["p"], tails)
                assert dims == case["pre"][tails][0] and wins == case["pre"][tails][1], (case["name"], tails)


def test_every_planted_value_is_there(oracle):
    for case in big_cases(oracle):
        n16 = 0
        for s in range(case["S"]):
            have = set(zip(case["test"][:, s].tolist(), case["ref"][:, s].tolist()))
            have16 = set(zip(case["test16"][:, s].tolist(), case["ref16"][:, s].tolist()))
            for tails in (0, 1):
                for v in tc.plant_values(case["pre"][tails][0][s], case["pre"][tails][1][s]):
                    assert v in have, (case["name"], s, v)
                    if max(v) <= 65535:
                        assert v in have16, (case["name"], s, v)
                        n16 += 1
        # the 16-bit matrix is the 32-bit one less what does not fit
        differ = (case["test"] != case["test16"]) | (case["ref"] != case["ref16"])
        assert ((case["test"][differ] > 65535) | (case["ref"][differ] > 65535) | (case["test"][differ] < 0)).all()
        assert case["test16"].min() >= 0 and max(case["test16"].max(), case["ref16"].max()) == 65535 and n16 > 0
        assert (case["test"] < 0).sum() == 1 and case["negative"] is not None


def test_plants_sit_on_the_edges_of_the_walk(oracle):
    """lane 0 and lane 63 of a block, the partial last block of a chromosome, a one-exon chromosome, the last block of a chunk and the first of
    the next, one of the last 16 blocks of a chunk: asserted from the restated grid, for every sample"""
    for case in big_cases(oracle):
        geo, sp = case["geo"], case["special"]
        blk = {k: int(geo.exon_block[e]) for k, e in sp.items()}
        lo, hi, _ = geo.blocks[blk["lane0"]]
        assert sp["lane0"] == lo and hi - lo == 64
        lo, hi, _ = geo.blocks[blk["lane63"]]
        assert sp["lane63"] == lo + 63
        lo, hi, c = geo.blocks[blk["partial_last_block"]]
        assert hi - lo < 64 and hi == case["chrom_off"][c + 1] and blk["partial_last_block"] > 0 and geo.blocks[blk["partial_last_block"] - 1][2] == c
        lo, hi, c = geo.blocks[blk["one_exon_chromosome"]]
        assert case["chrom_off"][c + 1] - case["chrom_off"][c] == 1
        assert geo.nsplit > 1
        a, b, f = blk["chunk_last_block"], blk["next_chunk_first_block"], blk["flush_block"]
        assert b == a + 1 and geo.chunk[b] == geo.chunk[a] + 1 and (b % geo.per) == 0
        end = geo.chunk_range(int(geo.chunk[f]))[1]
        assert end - tc.SM_WAVES <= f < end
        for s in range(case["S"]):
            assert case["planted"][list(sp.values()), s].all(), (case["name"], s)
        assert (0 in case["chrom_off"][1:] - case["chrom_off"][:-1])                # an empty chromosome
        assert {1, 63, 64, 65, 127, 129} <= set((case["chrom_off"][1:] - case["chrom_off"][:-1]).tolist())


def kind_facts(case, tails):
    dims, wins = case["pre"][tails][0], case["pre"][tails][1]
    return [(k[0], d, w) for k, d, w in zip(case["kinds"], dims, wins)]


def test_every_sample_kind_occurs(oracle):
    sets = [multi_cases(oracle)[0:1], multi_cases(oracle)[1:2], [cached("C0", lambda: tc.case_C(oracle, 0)), cached("C1", lambda: tc.case_C(oracle, 1))]]
    for group in sets:
        facts = [f for c in group for f in kind_facts(c, 1)]
        kinds = [c["kinds"] for c in group]
        # table samples: the four window relations
        tabs = [(d, w) for k, d, w in facts if k == "table"]
        assert all(d[0] > 0 and w[3] == 0 for d, w in tabs)
        assert any(w[0] == d[0] < 1024 for d, w in tabs) and any(w[0] == 1024 < d[0] for d, w in tabs)
        assert any(w[1] == d[1] for d, w in tabs) and any(w[1] < d[1] for d, w in tabs)
        # tail samples are tail samples in mode 2 (and table samples in mode 1, which has none)
        assert all(w[3] == 1 for k, d, w in facts if k == "tail") and any(k == "tail" for k, d, w in facts)
        assert all(w[3] == 0 for c in group for k, d, w in kind_facts(c, 0))
        # few reads, a finite N0, a sample without tables between two that have them
        assert all(d[0] > 0 and d[2] > 0 for k, d, w in facts if k == "few") and any(k == "few" for k, d, w in facts)
        assert any(d[0] > 0 and d[3] != tc.NO_N0 for k, d, w in facts if k == "n0")
        for c in group:
            f = kind_facts(c, 1)
            for s, (k, d, w) in enumerate(f):
                if k == "notab":
                    assert d[0] == 0 and d[3] in (1, 2) and 0 < s < c["S"] - 1 and f[s - 1][1][0] > 0 and f[s + 1][1][0] > 0
        assert any(k == "notab" for k, d, w in facts)
        del kinds
    # the limit of the tail search: where it reached 2^24 the served lengths add up to it
    lim = [d[0] + d[1] for c in big_cases(oracle) for k, d, w in kind_facts(c, 1) if w[3] == 1]
    assert lim and all(64 <= v <= tc.TAIL_MAX_COUNT for v in lim) and tc.TAIL_MAX_COUNT in lim


@pytest.mark.parametrize("E,S", tc.SMALL_SHAPES)
def test_small_cases_are_pinned_by_the_caps(oracle, E, S):
    case = tc.case_small(oracle, E, S)
    dims, wins, _ = tc.restate(oracle, case["test"], case["ref"], case["phi"], case["p"], 0, tc.SMALL_CAPS)
    assert all(d == (64, 64, 0, tc.NO_N0) for d in dims) and all(w == (64, 64, 128, 0) for w in wins)
    assert case["geo"].nsplit == 1 and case["planted"].sum() == min(E, 12) * S
    vals = set(zip(case["test"][case["planted"]].tolist(), case["ref"][case["planted"]].tolist()))
    assert vals <= {(o, r) for o in (0, 63, 64, 65) for r in (0, 63, 64, 65)} and (len(vals) == 12 or E * S < 12)


@pytest.mark.parametrize("S", [130, 257])
@pytest.mark.parametrize("caps", tc.PINNED_CAPS)
def test_pinned_lengths(oracle, S, caps):
    case = tc.case_pinned(oracle, S, caps)
    dims, wins = case["pre"][0][0], case["pre"][0][1]
    assert all(d[:2] == caps for d in dims), (dims[0], caps)
    assert tc.PINNED_LENGTHS == [1024, 1032, 4096, 4104, 5120, 5136, 8192, 12288]


def test_capacity_designs(oracle):
    base, designs = tc.capacity_designs(oracle)
    geo, per = base["geo"], base["per"]
    assert per == 64 and geo.nsplit == 16 and base["E"] * base["S"] <= 2 ** 20
    for name, (t, r, load, over) in designs.items():
        dims, wins, _ = tc.restate(oracle, t, r, base["phi"], base["p"], 1)
        assert dims[0] == base["dims"] and wins[0] == base["win"], name
        cold = ~tc.served_mask(t[:, 0], r[:, 0], dims[0])[:, None]
        loads = geo.list_loads(cold)
        assert loads.max() == load and (loads.max() > per) == over, (name, loads.max())
        assert (loads > 0).sum() == 1 and cold.sum() == load, name           # everything else is served
    t, r = designs["whole_block"][:2]
    e = np.flatnonzero(~tc.served_mask(t[:, 0], r[:, 0], base["dims"]))
    assert e.size == 64 and len(set(geo.exon_block[e])) == 1
    t, r = designs["whole_block_plus_one"][:2]
    b = sorted(set(geo.exon_block[np.flatnonzero(~tc.served_mask(t[:, 0], r[:, 0], base["dims"]))]))
    assert b[1] == b[0] + 16 and geo.chunk[b[0]] == geo.chunk[b[1]] and geo.wave[b[0]] == geo.wave[b[1]]
    t, r = designs["two_workgroups_one_over"][:2]
    b = sorted(set(geo.exon_block[np.flatnonzero(~tc.served_mask(t[:, 0], r[:, 0], base["dims"]))]))
    assert len(b) == 2 and geo.workgroup(0, int(geo.chunk[b[0]])) != geo.workgroup(0, int(geo.chunk[b[1]])) and geo.list_of(0, b[0]) == geo.list_of(0, b[1])


def planted_served(oracle, case, tails):
    """(sample, obs, ref, want [n][3], libm [n][3]) of the planted served cells of a case"""
    out = []
    dims, wins, shapes = case["pre"][tails]
    for s in range(case["S"]):
        e = np.flatnonzero(case["planted"][:, s])
        o, r = case["test"][e, s], case["ref"][e, s]
        ok = tc.served_mask(o, r, dims[s])
        if not ok.any():
            continue
        o, r = o[ok], r[ok]
        want, _ = tc.host_definition(oracle, shapes[s], o, r, wins[s])
        ell, _ = oracle.get_loglike_matrix(case["phi"][s], case["p"][s], o + r, o, 1.0, oracle.LIBM)
        out.append((s, o, r, want, ell))
    return out


def test_definition_and_reference_agree_on_the_planted_cells(oracle):
    """the host definition of every planted served cell within 1e-10 relative of the LIBM flavour; cells without reads are +0"""
    worst = {}
    for case in big_cases(oracle):
        for tails in (0, 1):
            n = 0
            for s, o, r, want, ell in planted_served(oracle, case, tails):
                ok = (want == ell) | (np.abs(want - ell) <= REL_TOL * np.abs(ell))
                assert ok.all(), (case["name"], tails, s, case["kinds"][s], o[~ok.all(axis=1)][:4], r[~ok.all(axis=1)][:4])
                zero = (o + r) == 0
                assert (want[zero] == 0).all() and not np.signbit(want[zero]).any()
                nz = ell != 0
                key = ("tail" if case["pre"][tails][1][s][3] else "table")
                worst[key] = max(worst.get(key, 0.0), float(np.max(np.abs(want[nz] - ell[nz]) / np.abs(ell[nz]))))
                n += o.size
            assert n > 20 * case["S"]
    print("\nhost definition against the LIBM flavour on the planted served cells, largest relative deviation: %s" % worst)
    assert set(worst) == {"tail", "table"}
