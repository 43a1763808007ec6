#!/usr/bin/env python3
"""
Generate tests/golden/*.npz by IMPORTING the reference's numpy half
(/root/reference: ssdutils.py, utils.py geometry, transforms.LabelCreatorTransform)
in the build container, with empty stub modules for cv2 / tensorflow / tqdm
(the hot-path functions never touch them).

Only data (inputs + expected outputs) is written.  The reference source never
travels.  Run:  python tools/make_golden.py   (needs /root/reference; numpy 2.2.6)

Every fixture is also cross-checked here against oracle/boxes.py, bit-exactly.
"""
import os
import sys
import types
import numpy as np

REF = '/root/reference'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, 'tests', 'golden')


def import_reference():
    for name in ('cv2', 'tensorflow', 'tqdm'):
        if name not in sys.modules:
            m = types.ModuleType(name)
            if name == 'tqdm':
                m.tqdm = object
            sys.modules[name] = m
    sys.path.insert(0, REF)
    import ssdutils, utils, transforms   # noqa
    return ssdutils, utils, transforms


def rand_gt(rng, n):
    w = rng.uniform(0.1, 0.6, n); h = rng.uniform(0.1, 0.6, n)
    cx = rng.uniform(w / 2, 1 - w / 2); cy = rng.uniform(h / 2, 1 - h / 2)
    return np.stack([cx, cy, w, h], 1), rng.integers(0, 20, n)


def synth_pred(rng, A, C=20, n_hot=300, logit_scale=1.0, cluster=0, bg=4.0):
    """SURVEY 8d config-5 distribution: N(0,1) logits, +4 on background,
    +8 on n_hot random (anchor, class) pairs; loc ~ N(0, 0.5).
    cluster>0: the hot anchors come in runs of `cluster` consecutive anchor
    indices sharing a class (neighbouring cells -> real NMS suppression)."""
    logits = rng.normal(0, logit_scale, (A, C + 1))
    logits[:, C] += bg
    if cluster:
        starts = rng.choice(A - cluster, n_hot // cluster, replace=False)
        hot = (starts[:, None] + np.arange(cluster)[None, :]).ravel()
        hcls = np.repeat(rng.integers(0, C, len(starts)), cluster)
        logits[hot, hcls] += 8 + rng.normal(0, 1, hot.size)
    else:
        hot = rng.choice(A, n_hot, replace=False)
        logits[hot, rng.integers(0, C, n_hot)] += 8
    e = np.exp(logits - logits.max(1, keepdims=True))
    p = (e / e.sum(1, keepdims=True)).astype(np.float32)
    loc = rng.normal(0, 0.1 if cluster else 0.5, (A, 4)).astype(np.float32)
    return np.concatenate([p, loc], 1)


def main():
    sys.path.insert(0, ROOT)
    from oracle import boxes as ob
    su, ut, tf = import_reference()
    os.makedirs(OUT, exist_ok=True)
    meta = dict(numpy=np.__version__)
    print('numpy', np.__version__)

    for pname in ('vgg300', 'vgg512'):
        preset = su.get_preset_by_name(pname)
        ref_anchors = su.get_anchors_for_preset(preset)
        A = len(ref_anchors)
        anch = np.array([[a.center.x, a.center.y, a.size.w, a.size.h] for a in ref_anchors])
        anch_abs = su.anchors2array(ref_anchors, ut.Size(1000, 1000))

        # ---- G1 anchors --------------------------------------------------
        o_anch = ob.anchors(ob.get_preset(pname))
        assert o_anch.shape == anch.shape and np.array_equal(o_anch, anch), 'G1 anchors'
        assert np.array_equal(ob.anchors_abs(o_anch), anch_abs), 'G1 abs'
        np.savez_compressed(os.path.join(OUT, f'g1_anchors_{pname}.npz'),
                            anchors=anch, anchors_abs=anch_abs.astype(np.int32))

        # ---- G2 IoU / overlap + G3 labels ---------------------------------
        rng = np.random.default_rng(7 if pname == 'vgg300' else 8)
        lab = tf.LabelCreatorTransform(preset=preset, num_classes=20)
        cases = []
        for ci in range(12):
            n = int(rng.integers(1, 6))
            g, c = rand_gt(rng, n)
            if ci == 1:    # a tiny box: no anchor above 0.5 -> no positive
                g[0] = [0.5, 0.5, 0.012, 0.011]
            if ci == 2:    # two near-identical boxes: same-anchor conflict
                g = np.concatenate([g, g[:1] + [0.004, 0.0, 0.0, 0.002]]); c = np.append(c, (c[0] + 1) % 20)
            if ci == 3:    # exact duplicate box, different class: tie keeps the earlier
                g = np.concatenate([g, g[:1]]); c = np.append(c, (c[0] + 3) % 20)
            if ci == 4:    # heavy overlap of large boxes
                g = np.array([[0.5, 0.5, 0.6, 0.6], [0.52, 0.5, 0.58, 0.62], [0.5, 0.47, 0.62, 0.6]]); c = np.array([3, 7, 11])
            cases.append((g, c))
        g2 = {}
        for ci, (g, c) in enumerate(cases):
            boxes = [ut.Box('x', int(ci_), ut.Point(float(b[0]), float(b[1])), ut.Size(float(b[2]), float(b[3])))
                     for b, ci_ in zip(g, c)]
            gt = ut.Sample('f', boxes, ut.Size(1000, 1000))
            _, vec, _ = lab(None, None, gt)
            o_vec = ob.encode_labels(g, c, ob.get_preset(pname), 20, o_anch, anch_abs)
            assert vec.dtype == np.float32 and np.array_equal(vec, o_vec), f'G3 case {ci}'
            pos = np.nonzero(vec[:, 20] == 0)[0]
            g2[f'gt_{ci}'] = g; g2[f'cls_{ci}'] = c.astype(np.int32)
            g2[f'pos_{ci}'] = pos.astype(np.int32); g2[f'rows_{ci}'] = vec[pos]
            # G2: raw overlap for the first box of each case
            ov = su.compute_overlap(su.box2array(boxes[0], ut.Size(1000, 1000)), anch_abs, 0.5)
            best, good, iou = ob.overlap(np.array(ob.prop2abs(*g[0]), np.float64), anch_abs, 0.5)
            assert (ov.best is None) == (best is None)
            if best is not None:
                assert ov.best.idx == best and ov.best.score == iou[best]
            assert [s.idx for s in ov.good] == list(good)
            g2[f'good_{ci}'] = np.array([s.idx for s in ov.good], np.int32)
            g2[f'goodiou_{ci}'] = np.array([s.score for s in ov.good], np.float64)
            g2[f'best_{ci}'] = np.array([-1 if ov.best is None else ov.best.idx], np.int32)
        g2['ncases'] = np.array([len(cases)])
        np.savez_compressed(os.path.join(OUT, f'g23_labels_{pname}.npz'), **g2)

        # ---- G4 decode + G5 NMS -------------------------------------------
        g4 = {}
        settings = [(0.5, 200, None), (0.5, None, 200), (0.01, None, 200), (0.3, 50, None)]
        rng = np.random.default_rng(11 if pname == 'vgg300' else 12)
        npred = 4
        for pi in range(npred):
            pred = synth_pred(rng, A, cluster=6 if pi == 3 else 0, bg=5.0 if (pi == 0 and pname == 'vgg300') else 7.0)
            if pi == 2:   # early-training style: huge offsets -> clamp at 100, boxes off-image
                pred[::97, 21:] *= 400
            # store sparsely: rows that can never reach the lowest threshold used are
            # replaced by a pure-background row at load time (tests/golden_util.py)
            keep_rows = np.nonzero(pred[:, :20].max(1) >= (0.009 if pi in (0, 3) else 0.25))[0]
            g4[f'predrows_{pi}'] = keep_rows.astype(np.int32)
            g4[f'predvals_{pi}'] = pred[keep_rows]
            bgrow = np.zeros(25, np.float32); bgrow[20] = 1
            dense = np.tile(bgrow, (A, 1)); dense[keep_rows] = pred[keep_rows]
            pred = dense
            for si, (thr, cap, max_out) in enumerate(settings):
                if thr == 0.01 and pi not in (0, 3):
                    continue
                while True:
                    p = pred.copy()
                    boxes = su.decode_boxes(p, ref_anchors, thr, {}, cap)
                    confs = np.array([b[0] for b in boxes], np.float32)
                    if len(np.unique(confs)) == len(confs):
                        break
                    assert thr < 0.3, 'fixture must avoid exact ties'
                    thr = round(thr * 1.5, 4)     # tie order is not contractual: move off it
                absb = np.array([ut.prop2abs(b[1].center, b[1].size, ut.Size(1000, 1000)) for b in boxes], np.int64).reshape(-1, 4)
                cls = np.array([b[1].labelid for b in boxes], np.int64)
                det = ob.decode(pred, o_anch, thr, cap)
                assert np.array_equal(det['conf'], confs), 'G4 conf'
                assert np.array_equal(det['cls'], cls), 'G4 cls'
                assert np.array_equal(ob.nms_roundtrip(det['box']), absb), 'G4 box'
                # the normalised integer box itself (before NMS's round trip):
                # recover from Box via exact abs2prop inverse check
                for k, b in enumerate(boxes):
                    cx, cy, w, h = ob.abs2prop(*det['box'][k])
                    assert (b[1].center.x, b[1].center.y, b[1].size.w, b[1].size.h) == (cx, cy, w, h), 'G4 prop'
                sel = su.suppress_overlaps(boxes)
                if max_out is not None:
                    sel = sel[:max_out]
                # identify survivors by (conf) which is unique
                pos = {float(c): k for k, c in enumerate(confs)}
                keep = np.array([pos[float(s[0])] for s in sel], np.int64)
                o_keep = ob.suppress(det, max_out)
                assert np.array_equal(keep, o_keep), 'G5 keep'
                tag = f'{pi}_{si}'
                g4[f'set_{tag}'] = np.array([thr, -1 if cap is None else cap, -1 if max_out is None else max_out], np.float64)
                g4[f'idx_{tag}'] = det['idx'].astype(np.int32)
                g4[f'cls_{tag}'] = cls.astype(np.int32)
                g4[f'conf_{tag}'] = confs
                g4[f'box_{tag}'] = det['box'].astype(np.int32)
                g4[f'nmsbox_{tag}'] = absb.astype(np.int32)
                g4[f'keep_{tag}'] = keep.astype(np.int32)
                print(pname, 'pred', pi, 'set', si, 'decoded', len(boxes), 'kept', len(keep))
        g4['npred'] = np.array([npred]); g4['nset'] = np.array([len(settings)])
        g4['A'] = np.array([A])
        np.savez_compressed(os.path.join(OUT, f'g45_detect_{pname}.npz'), **g4)

    # ---- G6 round-trip exceptions ------------------------------------------
    exc = []
    for xmin in range(0, 1000):
        xs = np.arange(xmin, 1000)
        for xmax in xs:
            c, s = ut.abs2prop(xmin, int(xmax), 0, 0, ut.Size(1000, 1000))
            r = ut.prop2abs(c, s, ut.Size(1000, 1000))
            if r[0] != xmin or r[1] != xmax:
                exc.append((xmin, int(xmax), r[0], r[1]))
    exc = np.array(exc, np.int32)
    a0 = np.repeat(np.arange(1000), 1)
    # oracle check over the full table
    xi, xa = np.triu_indices(1000)
    rt = ob.nms_roundtrip(np.stack([xi, xa, np.zeros_like(xi), np.zeros_like(xi)], 1))
    bad = (rt[:, 0] != xi) | (rt[:, 1] != xa)
    assert bad.sum() == len(exc), (bad.sum(), len(exc))
    assert np.array_equal(np.stack([xi[bad], xa[bad], rt[bad, 0], rt[bad, 1]], 1), exc)
    print('G6 exceptions', len(exc))
    np.savez_compressed(os.path.join(OUT, 'g6_roundtrip.npz'), exceptions=exc)

    # ---- G7 location encode/decode scalar pairs ----------------------------
    rng = np.random.default_rng(5)
    n = 256
    bx = np.stack([rng.uniform(0.1, 0.9, n), rng.uniform(0.1, 0.9, n), rng.uniform(0.05, 0.7, n), rng.uniform(0.05, 0.7, n)], 1)
    ax = np.stack([rng.uniform(0.1, 0.9, n), rng.uniform(0.1, 0.9, n), rng.uniform(0.05, 0.7, n), rng.uniform(0.05, 0.7, n)], 1)
    enc = np.zeros((n, 4)); dec = np.zeros((n, 4)); loc_in = rng.normal(0, 2, (n, 4)).astype(np.float32)
    loc_in[:8] = [[150, -3, 101, 2]] * 8      # > 100 clamp
    for i in range(n):
        # Python floats, as get_anchors_for_preset produces (np.float64 would not be 'weak')
        B = ut.Box('x', 0, ut.Point(*map(float, bx[i, :2])), ut.Size(*map(float, bx[i, 2:])))
        Aa = su.Anchor(ut.Point(*map(float, ax[i, :2])), ut.Size(*map(float, ax[i, 2:])), 0, 0, 0, 0)
        enc[i] = su.compute_location(B, Aa)
        assert np.array_equal(enc[i], ob.encode_location(bx[i], ax[i]))
        l = loc_in[i].copy()
        c, s = su.decode_location(l, Aa)
        l2 = loc_in[i].copy(); l2[l2 > 100] = 100
        x, y, w, h = ob.decode_location_np2(l2, ax[i])
        assert (float(c.x), float(c.y), s.w, s.h) == (float(x), float(y), w, h), 'G7 decode'
        assert type(c.x) is np.float32 and type(s.w) is float
        dec[i] = [c.x, c.y, s.w, s.h]
    np.savez_compressed(os.path.join(OUT, 'g7_location.npz'), box=bx, anchor=ax, enc=enc, loc=loc_in, dec=dec)
    # ---- G8 VOC07 11-point AP (average_precision.py; np.bool / np.int aliased for numpy >= 1.24) ----
    if not hasattr(np, 'bool'):
        np.bool = bool
    if not hasattr(np, 'int'):
        np.int = int
    import average_precision as apm
    from oracle import average_precision as oap
    rng = np.random.default_rng(21)
    g8 = {}
    for case in range(3):
        nimg = [6, 40, 15][case]
        calc = apm.APCalculator()
        db, dc, dk, ds, gb, gk, gs = [], [], [], [], [], [], []
        for img in range(nimg):
            ng = int(rng.integers(0, 5))
            gts = []
            for _ in range(ng):
                w, h = rng.uniform(0.1, 0.5, 2); cx = rng.uniform(w / 2, 1 - w / 2); cy = rng.uniform(h / 2, 1 - h / 2)
                k = int(rng.integers(0, 6 if case < 2 else 20))
                gts.append(ut.Box('c%d' % k, k, ut.Point(float(cx), float(cy)), ut.Size(float(w), float(h))))
                gb.append(ut.prop2abs(gts[-1].center, gts[-1].size, ut.Size(1000, 1000))); gk.append(k); gs.append(img)
            dets = []
            for g in gts:                       # jittered copies of the ground truth (some duplicated) + clutter
                for rep in range(int(rng.integers(0, 3))):
                    j = rng.normal(0, 0.03 if rep == 0 else 0.12, 4)
                    c = ut.Point(float(g.center.x + j[0]), float(g.center.y + j[1])); z = ut.Size(float(abs(g.size.w + j[2]) + 0.01), float(abs(g.size.h + j[3]) + 0.01))
                    dets.append((np.float32(rng.uniform(0.3, 1.0)), ut.normalize_box(ut.Box(g.label, g.labelid, c, z))))
            for _ in range(int(rng.integers(0, 4))):
                k = int(rng.integers(0, 8 if case < 2 else 20))
                w, h = rng.uniform(0.05, 0.5, 2)
                dets.append((np.float32(rng.uniform(0.05, 0.9)), ut.normalize_box(ut.Box('c%d' % k, k, ut.Point(float(rng.uniform(0.2, 0.8)), float(rng.uniform(0.2, 0.8))), ut.Size(float(w), float(h))))))
            calc.add_detections(gts, dets)
            for conf, b in dets:
                db.append(ut.prop2abs(b.center, b.size, ut.Size(1000, 1000))); dc.append(conf); dk.append(b.labelid); ds.append(img)
        assert len(set(np.float32(dc).tolist())) == len(dc), 'fixture must avoid exact confidence ties'
        aps = calc.compute_aps()
        ref_aps = {int(k[1:]): float(v) for k, v in aps.items()}
        mine = oap.compute_aps(np.array(db, np.float32).reshape(-1, 4), np.array(dc, np.float32), dk, ds, np.array(gb, np.float64).reshape(-1, 4), gk, gs)
        assert set(mine) == set(ref_aps) and all(mine[k] == ref_aps[k] for k in ref_aps), ('G8', case, mine, ref_aps)
        assert oap.aps2map(mine) == apm.APs2mAP(aps)
        g8[f'det_box_{case}'] = np.array(db, np.float32).reshape(-1, 4); g8[f'det_conf_{case}'] = np.array(dc, np.float32)
        g8[f'det_cls_{case}'] = np.array(dk, np.int32); g8[f'det_sample_{case}'] = np.array(ds, np.int32)
        g8[f'gt_box_{case}'] = np.array(gb, np.float64).reshape(-1, 4); g8[f'gt_cls_{case}'] = np.array(gk, np.int32); g8[f'gt_sample_{case}'] = np.array(gs, np.int32)
        g8[f'ap_cls_{case}'] = np.array(list(mine), np.int32); g8[f'ap_{case}'] = np.array([ref_aps[k] for k in mine], np.float64)
        g8[f'map_{case}'] = np.array([apm.APs2mAP(aps)], np.float64)
        print('G8 case', case, 'detections', len(dc), 'gt', len(gk), 'mAP', oap.aps2map(mine))
    g8['ncases'] = np.array([3])
    np.savez_compressed(os.path.join(OUT, 'g8_average_precision.npz'), **g8)

    # ---- G9 augmentation: the transforms that run without OpenCV, under the reference's own
    # `random` stream.  (a) geometry: RandomTransform(Expand) -> SamplePicker(7 samplers) on a coordinate image
    # (channel 0 = row, 1 = column), so the expand / crop window is read off the result; (b) pixels:
    # RandomTransform(Brightness) -> RandomTransform(Contrast) -> RandomTransform(ReorderChannels) on uint8 noise.
    import random as pyrandom
    from oracle import augment as oa

    def build_picker(trials):
        def sampler(ov):
            return tf.SamplerTransform(sample=True, min_scale=0.3, max_scale=1.0, min_aspect_ratio=0.5, max_aspect_ratio=2.0,
                                       min_jaccard_overlap=ov, max_trials=trials)
        return tf.SamplePickerTransform(samplers=[tf.SamplerTransform(sample=False)] + [sampler(o) for o in oa.SAMPLER_OVERLAPS[1:]])

    g9 = {}
    nrng = np.random.default_rng(99)
    ncase = 40
    tf_rnd_expand = tf.RandomTransform(prob=0.5, transform=tf.ExpandTransform(max_ratio=4.0, mean_value=[104, 117, 123]))
    picker = build_picker(50)
    n_exp = n_crop = n_drop = 0
    for case in range(ncase):
        size, boxes, cls = oa.synth_sample(nrng)
        gt = ut.Sample('x', [ut.Box('c%d' % c, c, ut.Point(b[0], b[1]), ut.Size(b[2], b[3])) for b, c in zip(boxes, cls)], ut.Size(*size))
        yy, xx = np.mgrid[0:size[1], 0:size[0]]
        img = np.stack([yy, xx, np.full_like(yy, 7)], -1).astype(np.int32)
        seed = 1000 + case
        pyrandom.seed(seed)
        d, _, g = tf_rnd_expand(img, None, gt)
        d, _, g = picker(d, None, g)
        # the same through the oracle
        rng = oa.new_rng(seed)
        ex = oa.plan_expand(rng, size, boxes, cls, 0.5)
        osz, ob_, oc_ = (size, boxes, cls) if ex is None else (ex[0], ex[3], ex[4])
        win, osz2, ob2, oc2 = oa.plan_sample_picker(rng, osz, ob_, oc_, 50)
        assert (g.imgsize.w, g.imgsize.h) == tuple(osz2) and d.shape[:2] == (osz2[1], osz2[0]), ('G9 size', case)
        rb = np.array([[b.center.x, b.center.y, b.size.w, b.size.h] for b in g.boxes], np.float64).reshape(-1, 4)
        assert np.array_equal(rb, np.array(ob2, np.float64).reshape(-1, 4)), ('G9 boxes', case)
        assert [b.labelid for b in g.boxes] == list(oc2), ('G9 classes', case)
        x0 = 0 if win is None else win[0]; y0 = 0 if win is None else win[2]
        exp_img = oa.expand(img, *ex[:3]) if ex is not None else img
        assert np.array_equal(np.asarray(d, np.float64), np.asarray(exp_img[y0:y0 + osz2[1], x0:x0 + osz2[0]], np.float64)), ('G9 window', case)
        n_exp += ex is not None; n_crop += win is not None; n_drop += len(oc2) < len(cls)
        g9[f'size_{case}'] = np.array(size, np.int32); g9[f'boxes_{case}'] = np.array(boxes, np.float64); g9[f'cls_{case}'] = np.array(cls, np.int32)
        g9[f'seed_{case}'] = np.array([seed]); g9[f'out_size_{case}'] = np.array([g.imgsize.w, g.imgsize.h], np.int32)
        g9[f'out_boxes_{case}'] = rb; g9[f'out_cls_{case}'] = np.array([b.labelid for b in g.boxes], np.int32)
        # where the result's corner pixels came from: (row, col) of the source image, or the mean value when expanded
        g9[f'corner00_{case}'] = np.asarray(d[0, 0], np.float64); g9[f'corner11_{case}'] = np.asarray(d[-1, -1], np.float64)
    print(f'G9 geometry: {ncase} cases, {n_exp} expanded, {n_crop} cropped, {n_drop} lost a box')
    tf_b = tf.RandomTransform(prob=0.5, transform=tf.BrightnessTransform(delta=32))
    tf_c = tf.RandomTransform(prob=0.5, transform=tf.ContrastTransform(lower=0.5, upper=1.5))
    tf_r = tf.RandomTransform(prob=0.5, transform=tf.ReorderChannelsTransform())
    npix = 16
    for case in range(npix):
        img = nrng.integers(0, 256, (20, 24, 3)).astype(np.uint8)
        seed = 5000 + case
        pyrandom.seed(seed)
        d = img
        for t in (tf_b, tf_c, tf_r):
            d, _, _ = t(d, None, None)
        rng = oa.new_rng(seed)
        o = img
        b_ = oa.plan_brightness(rng)
        if b_ is not None:
            o = oa.brightness(o, b_)
        c_ = oa.plan_contrast(rng)
        if c_ is not None:
            o = oa.contrast(o, c_)
        r_ = oa.plan_reorder(rng)
        if r_ is not None:
            o = o[:, :, r_]
        assert d.dtype == o.dtype and np.array_equal(d, o), ('G9 pixels', case)
        g9[f'pix_in_{case}'] = img; g9[f'pix_seed_{case}'] = np.array([seed]); g9[f'pix_out_{case}'] = np.asarray(d)
    g9['ncases'] = np.array([ncase]); g9['npix'] = np.array([npix])
    np.savez_compressed(os.path.join(OUT, 'g9_augment.npz'), **g9)
    # ---- G10 suppress_overlaps / non_maximum_suppression on arbitrary box lists (ssdutils.py:232-318) ----
    # lists that did not come out of decode_boxes: random boxes, several classes, any threshold.  Confidences are
    # distinct (the reference's order among exact ties is np.argsort's, i.e. unspecified).
    rng = np.random.default_rng(31)
    g10 = {}
    ncase = 10
    for case in range(ncase):
        n = int(rng.integers(1, 300))
        cx = rng.uniform(0.1, 0.9, n); cy = rng.uniform(0.1, 0.9, n)
        w = rng.uniform(0.05, 0.5, n); h = rng.uniform(0.05, 0.5, n)
        conf = rng.permutation(n).astype(np.float64) / n + rng.uniform(0, 0.4 / n, n)       # distinct also as float32
        conf = conf.astype(np.float32)
        assert len(set(conf.tolist())) == n
        lab = rng.integers(0, 5, n) * 3 - 2
        boxes = [(conf[i], ut.Box('c%d' % lab[i], int(lab[i]), ut.Point(float(cx[i]), float(cy[i])), ut.Size(float(w[i]), float(h[i]))))
                 for i in range(n)]
        sel = su.suppress_overlaps(boxes)
        keep = [next(i for i, bx in enumerate(boxes) if bx is s_) for s_ in sel]
        recs = [(float(c), b.labelid, tuple(int(v) for v in ut.prop2abs(b.center, b.size, ut.Size(1000, 1000)))) for c, b in boxes]
        assert ob.suppress_list(recs, 0.45) == keep, ('G10 suppress', case)
        thr = [0.3, 0.6, 0.05, 0.45, 0.9][case % 5]
        one = [i for i in range(n) if lab[i] == lab[0]]
        sel1 = su.non_maximum_suppression([boxes[i] for i in one], thr)
        keep1 = [next(k for k, i in enumerate(one) if boxes[i] is s_) for s_ in sel1]
        assert ob.nms_list([(recs[i][0], recs[i][2]) for i in one], thr) == keep1, ('G10 nms', case)
        g10[f'box_{case}'] = np.stack([cx, cy, w, h], 1); g10[f'conf_{case}'] = conf; g10[f'label_{case}'] = lab.astype(np.int32)
        g10[f'keep_{case}'] = np.array(keep, np.int32)
        g10[f'thr_{case}'] = np.array([thr]); g10[f'one_{case}'] = np.array(one, np.int32); g10[f'keep1_{case}'] = np.array(keep1, np.int32)
        print('G10 case', case, 'boxes', n, 'kept', len(keep), '| single class', len(one), 'thr', thr, 'kept', len(keep1))
    g10['ncases'] = np.array([ncase])
    np.savez_compressed(os.path.join(OUT, 'g10_nms_lists.npz'), **g10)
    print('all golden fixtures written and oracle agrees bit-exactly')


def main_c80():
    """G11 / G12: decode + NMS and labels at 80 classes (the wide kernels), same recipe as G45 / G23."""
    sys.path.insert(0, ROOT)
    from oracle import boxes as ob
    su, ut, tf = import_reference()
    C = 80
    for pname in ('vgg300', 'vgg512'):
        preset = su.get_preset_by_name(pname)
        ref_anchors = su.get_anchors_for_preset(preset)
        A = len(ref_anchors)
        anch_abs = su.anchors2array(ref_anchors, ut.Size(1000, 1000))
        o_anch = ob.anchors(ob.get_preset(pname))

        # ---- G12 labels: LabelCreatorTransform (compute_location) at 80 classes -----------------------------
        rng = np.random.default_rng(111 if pname == 'vgg300' else 112)
        lab = tf.LabelCreatorTransform(preset=preset, num_classes=C)
        g12 = {}
        ncase = 8
        for ci in range(ncase):
            n = int(rng.integers(1, 7))
            w = rng.uniform(0.1, 0.6, n); h = rng.uniform(0.1, 0.6, n)
            g = np.stack([rng.uniform(w / 2, 1 - w / 2), rng.uniform(h / 2, 1 - h / 2), w, h], 1)
            c = rng.integers(0, C, n)
            if ci == 0:
                c[0] = C - 1           # the highest class id
            boxes = [ut.Box('x', int(k), ut.Point(float(b[0]), float(b[1])), ut.Size(float(b[2]), float(b[3]))) for b, k in zip(g, c)]
            _, vec, _ = lab(None, None, ut.Sample('f', boxes, ut.Size(1000, 1000)))
            o_vec = ob.encode_labels(g, c, ob.get_preset(pname), C, o_anch, anch_abs)
            assert vec.dtype == np.float32 and vec.shape[1] == C + 5 and np.array_equal(vec, o_vec), f'G12 case {ci}'
            pos = np.nonzero(vec[:, C] == 0)[0]
            g12[f'gt_{ci}'] = g; g12[f'cls_{ci}'] = c.astype(np.int32)
            g12[f'pos_{ci}'] = pos.astype(np.int32); g12[f'rows_{ci}'] = vec[pos]
        g12['ncases'] = np.array([ncase]); g12['num_classes'] = np.array([C])
        np.savez_compressed(os.path.join(OUT, f'g12_labels_c80_{pname}.npz'), **g12)

        # ---- G11 decode_boxes + suppress_overlaps at 80 classes ----------------------------------------------
        g11 = {}
        settings = [(0.5, 200, None), (0.5, None, 200), (0.3, 50, None)]
        rng = np.random.default_rng(211 if pname == 'vgg300' else 212)
        npred = 3
        for pi in range(npred):
            pred = synth_pred(rng, A, C=C, n_hot=600 if pi == 1 else 300, cluster=6 if pi == 2 else 0, bg=7.0)
            keep_rows = np.nonzero(pred[:, :C].max(1) >= 0.25)[0]
            g11[f'predrows_{pi}'] = keep_rows.astype(np.int32)
            g11[f'predvals_{pi}'] = pred[keep_rows]
            bgrow = np.zeros(C + 5, np.float32); bgrow[C] = 1
            dense = np.tile(bgrow, (A, 1)); dense[keep_rows] = pred[keep_rows]
            pred = dense
            for si, (thr, cap, max_out) in enumerate(settings):
                while True:
                    boxes = su.decode_boxes(pred.copy(), ref_anchors, thr, {}, cap)
                    confs = np.array([b[0] for b in boxes], np.float32)
                    if len(np.unique(confs)) == len(confs):
                        break
                    assert thr < 0.9, 'fixture must avoid exact ties'
                    thr = round(thr * 1.2, 4)     # tie order is not contractual: move off it
                absb = np.array([ut.prop2abs(b[1].center, b[1].size, ut.Size(1000, 1000)) for b in boxes], np.int64).reshape(-1, 4)
                cls = np.array([b[1].labelid for b in boxes], np.int64)
                det = ob.decode(pred, o_anch, thr, cap)
                assert np.array_equal(det['conf'], confs) and np.array_equal(det['cls'], cls), 'G11 decode'
                assert np.array_equal(ob.nms_roundtrip(det['box']), absb), 'G11 box'
                sel = su.suppress_overlaps(boxes)
                if max_out is not None:
                    sel = sel[:max_out]
                pos = {float(c): k for k, c in enumerate(confs)}
                keep = np.array([pos[float(q[0])] for q in sel], np.int64)
                assert np.array_equal(keep, ob.suppress(det, max_out)), 'G11 keep'
                tag = f'{pi}_{si}'
                g11[f'set_{tag}'] = np.array([thr, -1 if cap is None else cap, -1 if max_out is None else max_out], np.float64)
                g11[f'idx_{tag}'] = det['idx'].astype(np.int32)
                g11[f'cls_{tag}'] = cls.astype(np.int32)
                g11[f'conf_{tag}'] = confs
                g11[f'box_{tag}'] = det['box'].astype(np.int32)
                g11[f'keep_{tag}'] = keep.astype(np.int32)
                print(pname, 'c80 pred', pi, 'set', si, 'decoded', len(boxes), 'kept', len(keep), 'classes', len(set(cls.tolist())))
        g11['npred'] = np.array([npred]); g11['nset'] = np.array([len(settings)])
        g11['A'] = np.array([A]); g11['num_classes'] = np.array([C])
        np.savez_compressed(os.path.join(OUT, f'g11_detect_c80_{pname}.npz'), **g11)


if __name__ == '__main__':
    if sys.argv[1:] == ['c80']:            # only the 80-class fixtures
        main_c80()
    else:
        main()
        main_c80()
