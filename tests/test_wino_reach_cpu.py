"""The launch decisions of the F(m,7) and F(4x4,3x3) convs restated on the host (tests/wino_reach.py) against the library's own
host-only rtpose_conv2d_winograd_fits, the tag of every Winograd case of the suite (tests/wino_cases.py) against that
restatement at 256 CUs, and the tables together against the REQUIRED set: every kernel instance the launchers can select is
launched by a case, with nothing exempted.  No GPU: the decisions are integer arithmetic."""
import itertools

import conv_slices as cs
import wino_cases as wc
import wino_reach as wr


# ---- the restatement against the library -------------------------------------------------------------------------------------
def _lib_fits(capi, d, k, m, cin, cout, n, h, w, pad_in, pool=0, relu=0, prelu=0):
    d[0].k, d[0].wino_m, d[0].cin, d[0].cout, d[0].pool, d[0].relu = k, m, cin, cout, pool, relu
    d[0].prelu = 1 << 12 if prelu else None          # (only tested against NULL on the host)
    d[0].lin = capi.Layout.padded(cin, h, w, pad_in)
    return capi.lib.rtpose_conv2d_winograd_fits(d, n, h, w)


def _threshold_widths(fm):
    """the widths at which the transform items per thread of a strip of whole rows go 1 -> 2 -> 3 (NI = ceil(rows * GX * 2 / 256)),
    where the strips turn from the flat space to strips per image (positions per image 255 / 256), and the LDS limit"""
    ws = set()
    for gx in range(1, 40):
        for rows_gx, lim in ((wr.strip_rows(gx) * gx * wr.CG, 256), (wr.strip_rows(gx) * gx * wr.CG, 512),
                             (2 * wr.strip_rows(gx) * wr.row_stride(gx, fm + 6) * 16, wr.LDS7)):
            nxt = wr.strip_rows(gx + 1) * (gx + 1) * wr.CG if lim != wr.LDS7 else 2 * wr.strip_rows(gx + 1) * wr.row_stride(gx + 1, fm + 6) * 16
            if rows_gx <= lim < nxt:
                ws |= {gx * fm, gx * fm + 1}          # the last width of gx groups per row, the first of gx + 1
    return sorted(ws)


def test_restated_fits_is_the_librarys(capi):
    d = (capi.ConvDesc * 1)()
    checked = {0: 0, 1: 0}
    ni_seen = {fm: set() for fm in (4, 6, 8)}

    def one(fm, cin, cout, n, h, w, pad_in, pool=0, prelu=0):
        want = wr.fits(7, fm, cin, cout, n, h, w, h + pad_in, pool, 0, prelu)
        got = _lib_fits(capi, d, 7, fm, cin, cout, n, h, w, pad_in, pool, 0, prelu)
        assert got == want, (fm, cin, cout, n, h, w, pad_in, pool, prelu, got, want)
        checked[want] += 1
        p = wr.plan7(n, h, w, h + pad_in, fm)
        if cin % 8 == 0 and cout > 0 and wr.cout_pad(cout) % 128 == 0:
            ni_seen[fm].add((min(p.ni, 3), bool(p.tpi), p.lds <= wr.LDS7))

    for fm in (4, 6, 8):
        # a broad grid: tiny to wide maps, one image and batches whose flat strips cross images, two paddings
        for n, h, w, pad_in in itertools.product((1, 2, 5), (1, 3, 6, 9, 20, 46), (1, 7, 20, 27, 46, 49, 80, 100, 130, 184), (3, 4)):
            one(fm, 16, 128, n, h, w, pad_in)
        # positions per image 255 / 256: H x GX around 256 with GX = 1 (W <= fm), 5, 8 and 17
        for gx, h in ((1, 255), (1, 256), (5, 51), (5, 52), (8, 31), (8, 32), (17, 15), (17, 16)):
            for n in (1, 3):
                one(fm, 16, 128, n, h, gx * fm, 3)
                one(fm, 16, 128, n, h, gx * fm - fm + 1, 3)
        # NI 1 -> 2 -> 3 and the LDS limit, per image (tall maps) and flat (short maps, with and without a crossing strip)
        for w in _threshold_widths(fm):
            for n, h in ((1, 46), (1, 4), (3, 4), (2, 9), (1, 300)):
                one(fm, 16, 128, n, h, w, 3)
                one(fm, 16, 128, n, h, w, 5)
        # cin and cout padding, the refusals
        for cin, cout in itertools.product((0, 4, 8, 12, 16, 24, 100, 128), (0, 1, 38, 64, 65, 100, 128, 129, 192, 193, 256, 384)):
            one(fm, cin, cout, 2, 20, 27, 3)
        one(fm, 16, 128, 1, 20, 27, 3, pool=1)
        one(fm, 16, 128, 1, 20, 27, 3, prelu=1)
    assert _lib_fits(capi, d, 7, 5, 16, 128, 1, 20, 27, 3) == 0 == wr.fits(7, 5, 16, 128, 1, 20, 27, 23)
    assert _lib_fits(capi, d, 7, 0, 16, 128, 1, 20, 27, 3) == 1 == wr.fits(7, 0, 16, 128, 1, 20, 27, 23)
    assert checked[0] > 300 and checked[1] > 1000, checked
    for fm in (4, 6, 8):   # the sweep saw NI 1 and 2 in both strip modes, NI 3, and (F(8,7)) a plan that fails on the LDS alone
        assert {(1, False, True), (1, True, True), (2, False, True), (2, True, True)} <= ni_seen[fm], (fm, ni_seen[fm])
        assert any(ni == 3 for ni, _, _ in ni_seen[fm]), (fm, ni_seen[fm])
    assert any(ni <= 2 and not lds for ni, _, lds in ni_seen[8]), ni_seen[8]
    # F(4x4,3x3): cin in whole 16-channel pairs of chunks, at least two; PReLU excludes ReLU and the fused pool
    for cin, cout in itertools.product((0, 8, 16, 24, 32, 40, 48, 64, 288), (0, 1, 24, 64, 100, 512)):
        for pool, relu, prelu in ((0, 1, 0), (1, 1, 0), (0, 0, 1), (0, 1, 1), (1, 0, 1)):
            want = wr.fits(3, 4, cin, cout, 2, 8, 8, 9, pool, relu, prelu)
            assert _lib_fits(capi, d, 3, 4, cin, cout, 2, 8, 8, 1, pool, relu, prelu) == want, (cin, cout, pool, relu, prelu)


def test_plan_thresholds_are_where_the_source_puts_them():
    """make_plan by hand at the thresholds the case tags lean on (csrc/conv_wino7.hip:930-960)"""
    p = wr.plan7(1, 32, 46, 35, 6)                   # 32 rows x 8 groups = 256 positions: strips per image
    assert (p.gx, p.tpi, p.mtiles, p.nrows, p.ni) == (8, 8, 8, wr.strip_rows(8), 1) and wr.strip_rows(8) == 11
    p = wr.plan7(3, 31, 46, 34, 6)                   # 248: one flat space, a strip reaches over the 3 gap rows into the next image
    assert (p.tpi, p.mtiles, p.crossing, p.nrows) == (0, 24, True, 3 + 3 + 7) and p.ni == 1
    assert wr.plan7(1, 20, 80, 23, 6).ni == 2 and wr.plan7(1, 20, 78, 23, 6).ni == 2 and wr.plan7(1, 20, 72, 23, 6).ni == 1
    assert wr.row_stride(8, 12) == 200 and wr.row_stride(6, 14) == 182 and wr.row_stride(12, 10) == 252
    assert wr.fits7(128, 128, 2, 184, 184, 187, 6) == 0 and wr.plan7(2, 184, 184, 187, 6).lds > wr.LDS7
    assert wr.grid_ids(63, 2) == (0, 126) and wr.grid_ids(65, 2) == (1, 144) and wr.grid_ids(300, 1) == (0, 300)


# ---- the tags ------------------------------------------------------------------------------------------------------------------
def test_every_case_tag_is_what_the_restated_launch_selects_at_256_cus():
    cases = wc.all_cases()
    assert len(cases) > 120
    wrong = [(where, g, tag, wc.tag_of(g)) for where, tag, g in cases if wc.tag_of(g) != tag]
    assert not wrong, wrong
    for where, tag, g in cases:
        assert wr.fits(g.k, g.m, g.cin, g.cout, g.n, g.h, g.w, g.h + g.pad_in, g.pool, 0, g.prelu) == 1, (where, g)


def test_the_slice_tables_winograd_rows_are_all_tagged():
    rows = [r for r in cs.TINY_F32 if (r[0], r[1]) in ((3, 4), (7, 4), (7, 6), (7, 8))]
    rows += [r for r in cs.LARGE_F32 if (r[0], r[1]) in ((3, 4), (7, 4), (7, 6), (7, 8))]
    assert len(rows) == 11 and set(rows) == set(wc.SLICES)
    for row, tags in wc.SLICES.items():   # the F(m,7) rows of LARGE_F32 run with and without a scratch
        assert len(tags) == (2 if (row in cs.LARGE_F32 and row[0] == 7) else 1)


def test_new_cases_each_add_a_launch_no_earlier_table_has():
    """tests/test_wino_reach_gpu.py is the smallest set that fills the gaps: every one of its tags is new (the ragged-cout case
    apart, which repeats an instance on purpose)."""
    old = {tag for where, tag, _ in wc.all_cases() if not where.startswith("REACH")}
    new7 = [tag for tag, row in wc.REACH7 if row[4] % 128 == 0]
    assert not set(new7) & old and len(set(new7)) == len(new7)
    # F(4x4,3x3): the tag and whether the persistent launch comes out as whole rounds
    def kind(tag, g):
        return tag, wr.reach4(g.n, g.h, g.w, g.cin, g.cout, g.groups, wr.CUS, g.prelu).whole
    # (CLAMP_CASES has launched 'plain<=CUs' before, in a test of the buffer descriptors that compares with fp32 conv2d only:
    # no float64 reference, no bit identity with the small form)
    old4 = {kind(tag, g) for where, tag, g in wc.all_cases() if not where.startswith(("REACH", "CLAMP")) and g.k == 3}
    new4 = [kind(tag, g) for where, tag, g in wc.all_cases() if where == "REACH4"]
    assert not set(new4) & old4 and len(set(new4)) == len(new4) == len(wc.REACH4)


# ---- REQUIRED --------------------------------------------------------------------------------------------------------------------
def test_required_7x7_launches_are_all_reached():
    tags = {tag for _, tag, g in wc.all_cases() if g.k == 7}
    req, either = wc.required7()
    assert len(req) == 4 + 3 * 5 and len(either) == 3 * (5 + 2 * 3)
    # spelled out for F(6,7): the names are the kernel templates of csrc/conv_wino7.hip
    assert {r for r in req if ",6,2>" in r or ",6,1>" in r or "wino7s" in r} == {
        "wino7s_f32<1> image plain", "wino7s_f32<1> flat plain", "wino7s_f32<2> image plain", "wino7s_f32<2> flat plain",
        "wino7_f32<1,8,6,2> image persistent", "wino7_f32<1,0,6,2> flat persistent", "wino7_f32<1,0,6,2> image persistent",
        "wino7_f32<2,0,6,1> flat persistent", "wino7_f32<2,0,6,1> image persistent"}
    assert ("wino7_f32<1,8,6,2> image plain", "wino7_f32<1,8,6,2> image plain+remap") in either       # either block order ...
    assert ("wino7_f32<1,8,6,2> image plain",) in either and ("wino7_f32<1,8,6,2> image plain+remap",) in either   # ... and both
    assert ("wino7_f32<2,0,8,1> flat plain+remap", "wino7_f32<2,0,8,1> image plain+remap") in either
    assert "wino7_f32<1,12,4,1> image persistent" in req and "wino7_f32<1,6,8,1> image persistent" in req
    assert not req - tags, "never launched: %s" % sorted(req - tags)
    missing = [e for e in either if not set(e) & tags]
    assert not missing, "never launched: %s" % missing
    # and the dispatch returns nothing REQUIRED does not name: every tag of a sweep is one of its words
    names = req | {t for e in either for t in e}
    for fm in (4, 6, 8):
        for n, h, w, (cout, groups), scratch in itertools.product((1, 2, 7, 23, 64), (1, 5, 20, 46), (7, 27, 46, 49, 80, 100),
                                                                   ((128, 1), (256, 2), (384, 2)), (True, False)):
            if wr.fits7(16, cout, n, h, w, h + 3, fm):
                assert wr.tag7(wr.reach7(n, h, w, 16, cout, groups, h + 3, fm, wr.CUS, scratch)) in names, (fm, n, h, w, cout, groups)


def _words(tag):
    shape, _, rest = tag.partition(" ")
    return shape, set(rest.split())


def test_required_4x4_launch_shapes_are_all_reached():
    have = [_words(tag) for _, tag, g in wc.all_cases() if g.k == 3]
    assert {s for s, _ in have} == set(wr.SHAPES4)
    missing = []
    for shape, word in wc.required4():
        if word is None:
            ok = any(s == shape and "prelu" not in ws for s, ws in have)
        else:
            ok = any(s == shape and word in ws for s, ws in have)
        if not ok:
            missing.append((shape, word))
    assert len(wc.required4()) == 18 and not missing, "never launched: %s" % missing
    # both kinds of a persistent launch without a second one: whole rounds, and a last round more than half full
    whole = {wr.reach4(g.n, g.h, g.w, g.cin, g.cout, g.groups, wr.CUS, g.prelu).whole
             for _, tag, g in wc.all_cases() if g.k == 3 and _words(tag)[0] == "persistent"}
    assert whole == {True, False}


def test_edges_the_tables_cover():
    """what the free-text comments of the tables used to promise: every W modulo 6 of F(6,7), one chunk and several, strips that
    cross images and ragged last strips in every form, a gap wider than the padding, ragged cout, two branches"""
    seen = {4: set(), 6: set(), 8: set(), 3: set()}
    for _, _, g in wc.all_cases():
        if g.k == 7:
            seen[g.m or 6] |= wr.edges7(g.n, g.h, g.w, g.cin, g.cout, g.groups, g.pad_in, g.m or 6)
        else:
            seen[3] |= wr.edges4(g.n, g.h, g.w, g.cin, g.cout, g.groups, g.pad_in)
    for fm in (4, 6, 8):
        assert {"chunks", "one chunk", "ragged last strip", "strip crosses images", "two branches"} <= seen[fm], (fm, seen[fm])
        assert not any("H<strip rows" in s for s in seen.values())
    assert {"W%%6=%d" % r for r in range(6)} | {"gap>padding", "ragged cout"} <= seen[6]
    assert {"W%%4=%d" % r for r in range(4)} <= seen[4] and len([e for e in seen[8] if e.startswith("W%8")]) >= 6
    assert {"H%%4=%d" % r for r in range(4)} | {"W%%4=%d" % r for r in range(4)} | {"gap>padding", "ragged cout", "tile crosses images",
                                                                                  "two branches"} <= seen[3]
    assert wr.edges7(1, 9, 80, 8, 128, 1, 4, 6) == {"W%6=2", "one chunk", "gap>padding"}
    assert wr.edges7(3, 23, 18, 64, 256, 1, 3, 6) == {"W%6=0", "chunks", "strip crosses images"}


def test_reach_follows_the_cu_count():
    """the same geometry on another device selects another launch: the GPU cases ask for their reach on the device they run on"""
    assert wr.tag7(wr.reach7(12, 46, 46, 128, 128, 2, 49, 6, 256)).endswith("persistent")
    assert wr.tag7(wr.reach7(12, 46, 46, 128, 128, 2, 49, 6, 304)).endswith("plain+remap")
    assert wr.tag7(wr.reach7(12, 46, 46, 128, 128, 2, 49, 6, 288)).endswith("plain+remap")     # whole rounds: one block per tile
    assert wr.tag7(wr.reach7(2, 46, 46, 128, 128, 1, 49, 6, 40)) == "wino7_f32<1,8,6,2> image plain"
    assert wr.reach4(20, 46, 46, 32, 192, 1, 256).shape == "plain>CUs" and wr.reach4(20, 46, 46, 32, 192, 1, 240).shape == "persistent+small"
