"""Hand cases of the 'paper' matching rule for vgg300, shared by the CPU and GPU tests:
(name, boxes as (cx, cy, w, h), the bipartite stage's {box: anchor}).  The expected matchings were worked out with a
prototype of the rule when the rule was written down; tests/test_match_ref.py pins the oracle on them."""

HAND_CASES = [
    # two boxes want anchor 7761: the lower box gets it, the other its next best
    ('identical', [(.5, .5, .3, .3), (.5, .5, .3, .3)], {0: 7761, 1: 7762}),
    # the pair of greatest IoU first: box 2 fits 7761 best, then box 0, then box 1
    ('nested', [(.5, .5, .30, .30), (.5, .5, .31, .31), (.5, .5, .29, .29)], {2: 7761, 0: 7762, 1: 7780}),
    # a shifted box overtakes the identical ones for the second anchor
    ('chain', [(.5, .5, .3, .3), (.5, .5, .3, .3), (.5, .5, .3, .3), (.52, .5, .3, .3)], {0: 7761, 3: 7762, 1: 7780, 2: 7742}),
    # 6, 6 and 5 anchors tie exactly for each box's best: the anchor tie rule decides; no box reaches IoU 0.5
    ('tiny boxes in one cell', [(.303, .303, .02, .02), (.305, .305, .03, .03), (.31, .30, .025, .02)], {1: 1871, 2: 1874, 0: 1875}),
    ('box beyond the image', [(1.2, 1.2, .05, .05)], {0: 8691}),
    ('no boxes', [], {}),
]
