"""Census of inter prediction cases, from what a decoder PARSED (the oracle's macroblocks(): y_mode, ref_frame, mv, uv_mv,
split_partition, has_nonzero, block_nonzero) and the frame geometry -- not from what tools/vp8_synth.py meant to write: NEAREST
and NEAR vectors are clamped by the decoder, and what counts is what is decoded.

Footprints follow the reference's semantics (prediction.cc:813-971): block origin + (vector >> 3), taps -2 .. +3 around every
pixel of the block, coordinates clamped to the padded plane.  A 16x16 luma block reads columns x0 + (mvx >> 3) - 2 .. + 18, an
8x8 chroma block 13 columns with the derived vector, a 4x4 SPLITMV unit 9.  d is the signed distance between the footprint's
outermost line and the plane's outermost line on that side; d >= 0: inside.  A footprint "beyond" an edge has no line inside
the plane at all: every sample clamps to the plane's outermost line.

Classes are plain strings; FULL[builder] is what the directed streams of tools/vp8_synth.py promise, EXCUSED[(builder, size)]
what a builder cannot reach at one size, with the reason -- and test_motion_streams.py checks that another size reaches it.
Test tooling only."""
import re

NEARESTMV, NEWMV, SPLITMV, B_PRED = 5, 8, 9, 4
EDGES = ("left", "right", "top", "bottom")
SPLIT_GROUPS = [(0, 1, 4, 5), (2, 3, 6, 7), (8, 9, 12, 13), (10, 11, 14, 15)]


def _distances(x_lo, y_lo, span, w, h):
    return {"left": x_lo, "right": w - 1 - (x_lo + span), "top": y_lo, "bottom": h - 1 - (y_lo + span)}


def _edge_classes(prefix, plane, d, span, reach):
    out = set()
    for e in EDGES:
        if -reach <= d[e] <= reach:
            out.add("%s/%s/%s/d=%+d" % (prefix, plane, e, d[e]))
    if prefix == "edge":
        beyond = {e: d[e] < -span for e in EDGES}
        for e in EDGES:
            if beyond[e]:
                out.add("edge/%s/%s/beyond" % (plane, e))
        for name, a, b in (("tl", "left", "top"), ("tr", "right", "top"), ("bl", "left", "bottom"), ("br", "right", "bottom")):
            if beyond[a] and beyond[b]:
                out.add("edge/%s/corner-%s/beyond" % (plane, name))
    return out


def classify_macroblock(o, col, row, mbw, mbh):
    """One record of the oracle's -> dict: kind ("intra" | "bpred" | "whole" | "split"), the vectors, fractions, distances, classes."""
    pw, ph, cw, ch = mbw * 16, mbh * 16, mbw * 8, mbh * 8
    rec = {"col": col, "row": row, "mode": int(o["y_mode"]), "ref": int(o["ref_frame"]), "classes": set()}
    if rec["ref"] == 0:
        rec["kind"] = "bpred" if rec["mode"] == B_PRED else "intra"
        return rec
    has_nz, y2_nz = bool(o["has_nonzero"]), bool(o["block_nonzero"][24])
    rec["coeffs"] = "none" if not has_nz else ("y2" if y2_nz else "ac")
    cls = rec["classes"]
    if rec["mode"] != SPLITMV:
        rec["kind"] = "whole"
        mvx, mvy = (int(v) for v in o["mv"][0]); cmx, cmy = (int(v) for v in o["uv_mv"][0])
        rec["mv"], rec["uv_mv"] = (mvx, mvy), (cmx, cmy)
        rec["luma_frac"], rec["chroma_frac"] = (mvx & 7, mvy & 7), (cmx & 7, cmy & 7)
        lx, ly = 16 * col + (mvx >> 3) - 2, 16 * row + (mvy >> 3) - 2
        cx, cy = 8 * col + (cmx >> 3) - 2, 8 * row + (cmy >> 3) - 2
        dl, dc = _distances(lx, ly, 20, pw, ph), _distances(cx, cy, 12, cw, ch)
        rec["d"] = {"luma": dl, "chroma": dc}
        rec["origin&3"] = {"luma": lx & 3, "chroma": cx & 3}
        li, ci = min(dl.values()) >= 0, min(dc.values()) >= 0
        rec["inside"] = {"luma": li, "chroma": ci}
        if li and ci:
            cls.add("frac/chroma=%d,%d" % rec["chroma_frac"])
            cls.add("frac/luma-x=%d/origin&3=%d" % (mvx & 7, lx & 3))
            cls.add("frac/chroma-x=%d/origin&3=%d" % (cmx & 7, cx & 3))
        cls |= _edge_classes("edge", "luma", dl, 20, 8) | _edge_classes("edge", "chroma", dc, 12, 8)
        if li and not ci: cls.add("edge/luma-inside+chroma-outside")
        if ci and not li: cls.add("edge/luma-outside+chroma-inside")
    else:
        rec["kind"] = "split"
        rec["partition"] = int(o["split_partition"])
        mvs = [tuple(int(v) for v in m) for m in o["mv"]]; uvs = [tuple(int(v) for v in m) for m in o["uv_mv"]]
        rec["mv"], rec["uv_mv"] = mvs, uvs
        rec["luma_frac"] = [(x & 7, y & 7) for x, y in mvs]; rec["chroma_frac"] = [(x & 7, y & 7) for x, y in uvs]
        cls.add("split/partition=%d" % rec["partition"])
        if rec["partition"] == 3 and len(set(rec["luma_frac"])) == 16:
            cls.add("split/16-fraction-pairs")
        for g in SPLIT_GROUPS:
            four = [mvs[b] for b in g]
            if len(set(four)) == 4:
                for s in (sum(v[0] for v in four), sum(v[1] for v in four)):
                    if s: cls.add("split/chroma-sum/%s/res=%d" % ("+" if s > 0 else "-", abs(s) & 7))
        inside, units = [], []
        for u in range(16):
            d = _distances(16 * col + 4 * (u & 3) + (mvs[u][0] >> 3) - 2, 16 * row + 4 * (u >> 2) + (mvs[u][1] >> 3) - 2, 8, pw, ph)
            cls |= _edge_classes("split", "luma", d, 8, 4); inside.append(min(d.values()) >= 0); units.append(d)
        for b in range(4):
            d = _distances(8 * col + 4 * (b & 1) + (uvs[b][0] >> 3) - 2, 8 * row + 4 * (b >> 1) + (uvs[b][1] >> 3) - 2, 8, cw, ch)
            cls |= _edge_classes("split", "chroma", d, 8, 4); units.append(d)
        rec["d"] = units; rec["inside"] = {"luma": all(inside), "luma units": inside}
        if inside.count(False) == 1: cls.add("split/one-unit-outside")
    return rec


def _quad_classes(slots, mbw, last_partial):
    """slots: the records of macroblocks 4 q .. 4 q + 3 (fewer in the frame's last quad)."""
    out = set()
    whole = [s for s in slots if s["kind"] == "whole"]
    lw = lambda s: s["luma_frac"] == (0, 0)
    cw_ = lambda s: s["chroma_frac"] == (0, 0)
    if len(slots) == 4 and len(whole) == 4:
        if all(lw(s) and cw_(s) for s in slots): out.add("wave/a-all-whole-pel")
        frac = [k for k, s in enumerate(slots) if not lw(s)]
        if len(frac) == 1 and all(lw(s) and cw_(s) for k, s in enumerate(slots) if k != frac[0]):
            out.add("wave/b-one-fractional/slot=%d" % frac[0])
        if all(s["mv"][0] % 16 == 8 and s["mv"][1] % 16 == 0 for s in slots): out.add("wave/c-luma-whole-chroma-fractional/x")
        if all(s["mv"][0] % 16 == 0 and s["mv"][1] % 16 == 8 for s in slots): out.add("wave/c-luma-whole-chroma-fractional/y")
    if any(s["luma_frac"][0] and not s["luma_frac"][1] for s in whole) and any(s["luma_frac"][1] and not s["luma_frac"][0] for s in whole):
        out.add("wave/d-x-only+y-only")
    # the wave-wide decisions: a plane that no slot filters is copied (by the slot's window alignment); a fraction in one axis only
    both = lambda s: s["inside"]["luma"] and s["inside"]["chroma"]
    if whole and all(lw(s) for s in whole):
        out |= {"wave/copy-luma/origin&3=%d" % s["origin&3"]["luma"] for s in whole if both(s)}
    if whole and all(cw_(s) for s in whole):
        out |= {"wave/copy-chroma/origin&3=%d" % s["origin&3"]["chroma"] for s in whole if both(s)}
    if any(s["luma_frac"][0] for s in whole) and not any(s["luma_frac"][1] for s in whole): out.add("wave/x-fraction-only")
    if any(s["luma_frac"][1] for s in whole) and not any(s["luma_frac"][0] for s in whole): out.add("wave/y-fraction-only")
    kinds = {s["kind"] for s in slots}
    if kinds == {"intra", "bpred", "split", "whole"}: out.add("wave/e-intra+bpred+split+whole")
    if last_partial and whole: out.add("wave/f-last-partial-quad")
    if len({s["row"] for s in whole}) == 2: out.add("wave/g-straddles-rows")
    ins = [s["inside"]["luma"] and s["inside"]["chroma"] for s in whole]
    if True in ins and False in ins: out.add("wave/h-inside+clamped")
    if {s["ref"] for s in whole} == {1, 2, 3}: out.add("wave/i-three-references")
    if {s["coeffs"] for s in whole} == {"none", "ac", "y2"}: out.add("wave/j-none+ac+y2")
    return out


class FrameCensus:
    def __init__(self, om):
        self.mbh, self.mbw = om.shape
        mbw, mbh = self.mbw, self.mbh
        self.records = [classify_macroblock(om[i // mbw, i % mbw], i % mbw, i // mbw, mbw, mbh) for i in range(mbw * mbh)]
        total = mbw * mbh
        self.quads = []
        for q in range((total + 3) // 4):
            slots = self.records[4 * q:4 * q + 4]
            qc = _quad_classes(slots, mbw, len(slots) < 4)
            self.quads.append(qc)
            for k, s in enumerate(slots):
                s["quad"], s["slot"] = q, k
        self.classes = set().union(*[r["classes"] for r in self.records], *self.quads)
        kinds = [r["kind"] for r in self.records]
        if "split" in kinds and "whole" not in kinds: self.classes.add("frame/split-only-inter")
        if "whole" in kinds and "split" not in kinds: self.classes.add("frame/no-split")
        border = [r for r in self.records if r["kind"] == "whole" and (r["col"] in (0, mbw - 1) or r["row"] in (0, mbh - 1))]
        self.edge_fractional_both = sum(1 for r in border if r["luma_frac"][0] and r["luma_frac"][1])
        self.edge_whole_pel = sum(1 for r in border if r["luma_frac"] == (0, 0))

    def macroblock_classes(self, i):
        """Classes of macroblock i: its own and its quad's."""
        return self.records[i]["classes"] | self.quads[i // 4]

    def describe(self, i):
        r = self.records[i]
        if r["kind"] in ("intra", "bpred"):
            return "mb %d (%d,%d) slot %d of quad %d: %s mode %d" % (i, r["col"], r["row"], r["slot"], r["quad"], r["kind"], r["mode"])
        s = "mb %d (%d,%d) slot %d of quad %d: %s mode %d ref %d coeffs %s mv %r chroma mv %r fractions luma %r chroma %r" % (
            i, r["col"], r["row"], r["slot"], r["quad"], r["kind"], r["mode"], r["ref"], r["coeffs"], r["mv"], r["uv_mv"], r["luma_frac"], r["chroma_frac"])
        if r["kind"] == "whole":
            s += " origin&3 %r %s d luma %r chroma %r" % (r["origin&3"], ", ".join("%s %s" % (p, "inside" if v else "clamped") for p, v in r["inside"].items()), r["d"]["luma"], r["d"]["chroma"])
        else:
            s += " partitioning %d luma units inside %r" % (r["partition"], r["inside"]["luma units"])
        return s

    def summary(self, i):
        """The short class line of a macroblock: what a failure message counts macroblocks by."""
        r = self.records[i]
        if r["kind"] != "whole":
            return r["kind"]
        others = [s for s in self.records[4 * r["quad"]:4 * r["quad"] + 4] if s is not r]
        fl = lambda s: "whole-pel" if s["luma_frac"] == (0, 0) else "fractional"
        fc = lambda s: "whole-pel" if s["chroma_frac"] == (0, 0) else "fractional"
        nb = "filtering" if any(s["kind"] == "whole" and (s["luma_frac"] != (0, 0) or s["chroma_frac"] != (0, 0)) for s in others) else "no filtering"
        return "%s-luma / %s-chroma, %s, in a quad with %s neighbour" % (fl(r), fc(r), "inside" if r["inside"]["luma"] and r["inside"]["chroma"] else "clamped", nb)


def stream_census(oracle_mbs):
    """oracle_mbs: macroblocks() of every INTER frame of a stream -> (classes, [FrameCensus])."""
    frames = [FrameCensus(om) for om in oracle_mbs]
    return set().union(*[f.classes for f in frames]), frames


def _d_classes(prefix, reach):
    return {"%s/%s/%s/d=%+d" % (prefix, p, e, d) for p in ("luma", "chroma") for e in EDGES for d in range(-reach, reach + 1)}


FULL = {
    "fraction": {"frac/chroma=%d,%d" % (a, b) for a in range(8) for b in range(8)}
                | {"frac/luma-x=%d/origin&3=%d" % (f, k) for f in (0, 2, 4, 6) for k in range(4)}
                | {"frac/chroma-x=%d/origin&3=%d" % (f, k) for f in range(8) for k in range(4)},
    "edge": _d_classes("edge", 8)
            | {"edge/%s/%s/beyond" % (p, e) for p in ("luma", "chroma") for e in EDGES + ("corner-tl", "corner-tr", "corner-bl", "corner-br")}
            | {"edge/luma-inside+chroma-outside"},
    "wave": {"wave/a-all-whole-pel", "wave/c-luma-whole-chroma-fractional/x", "wave/c-luma-whole-chroma-fractional/y", "wave/d-x-only+y-only",
             "wave/e-intra+bpred+split+whole", "wave/f-last-partial-quad", "wave/g-straddles-rows", "wave/h-inside+clamped",
             "wave/i-three-references", "wave/j-none+ac+y2", "wave/x-fraction-only", "wave/y-fraction-only"}
            | {"wave/b-one-fractional/slot=%d" % k for k in range(4)} | {"wave/copy-%s/origin&3=%d" % (p, k) for p in ("luma", "chroma") for k in range(4)},
    # vectors are always even (the bitstream carries mv / 2), so a sum of four is even: residues 1, 3, 5, 7 cannot occur in any
    # stream; test_gpu_stages.py runs chroma_mv over every integer sum instead
    "split": {"split/partition=%d" % p for p in range(4)} | {"split/16-fraction-pairs", "split/one-unit-outside", "frame/split-only-inter", "frame/no-split"}
             | {"split/chroma-sum/%s/res=%d" % (s, r) for s in "+-" for r in (0, 2, 4, 6)} | _d_classes("split", 4),
}
# "edge/luma-outside+chroma-inside" is promised by nobody: it cannot be (see motion_edge_stream's docstring)

# what a builder cannot reach at a size: (pattern, reason).  Everything excused here is reached at another size (asserted).
_ONE_MB = "one macroblock per frame: the stream's 11 inter frames hold the all-clamped cases and a few vectors; the sweep is at 80x48"
EXCUSED = {
    ("edge", (16, 16)): [(r"edge/(luma|chroma)/\w+/d=.*", _ONE_MB),
                         (r"edge/luma-inside\+chroma-outside", "the luma footprint (21 lines) is larger than the 16-pixel plane: luma is never inside")],
    ("edge", (33, 17)): [(r"edge/chroma/(left|right)/d=-[678]", "two macroblocks per border column and frame: 11 frames hold the first 22 of the 25 vectors of a side")],
    ("edge", (144, 16)): [(r"edge/(luma|chroma)/(left|right)/d=.*", "one macroblock per border column and frame: 11 frames hold 11 of the 25 vectors of a side"),
                          (r"edge/luma-inside\+chroma-outside", "the luma footprint (21 lines) is larger than the 16-pixel plane height: luma is never inside")],
    ("split", (16, 16)): [(r"split/partition=[012]", _ONE_MB.replace("80x48", "112x80")), (r"split/chroma-sum/.*", _ONE_MB.replace("80x48", "112x80")),
                          (r"split/chroma/\w+/d=\+4", _ONE_MB.replace("80x48", "112x80"))],
}


def promised(builder, size):
    rules = EXCUSED.get((builder, size), [])
    return {c for c in FULL[builder] if not any(re.fullmatch(p, c) for p, _ in rules)}
