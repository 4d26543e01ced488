"""The case table of the body-conv dispatch tests: tests/test_conv_dispatch_host.py proves on the CPU (with
tools/conv_plan_check --rules / --block) that it reaches every rule of csrc/conv_plan.h body_conv_rule that some input
up to 2048 x 2048 reaches, tests/test_gpu_conv_dispatch.py runs it on the GPU.

A frame of 3125 = 25 x 125 pixels (tile_rows = 50,000) is the smallest on the large side of the table's one map-size
threshold, 44 x 71 = 3124 the largest on the small side; 8 x 17 = 136 rows sits just above the strip kernel's 128-row
minimum and 7 x 18 = 126 just below it.  Stride-2 blocks list the input: (49, 249) and (50, 249) give 25 x 125,
(87, 141) and (88, 142) give 44 x 71; the odd ones read the bottom / right padding in the last output row / column.
"""

# (layer, block, (h, w) of the block's input) -> the rules of its conv1 and conv2
BLOCK_CASES = [
    ((3, 1, (25, 125)), ("strip_128x128", "strip_128x128")),
    ((3, 1, (44, 71)), ("strip_64x128", "strip_64x128")),
    ((3, 1, (8, 17)), ("strip_64x128", "strip_64x128")),
    ((3, 0, (49, 249)), ("r3_body", "r3_body")),
    ((3, 0, (88, 142)), ("h3_128x128", "h3_128x128")),
    ((4, 1, (25, 125)), ("strip_128x128_ks2", "strip_128x128_ks2")),
    ((4, 1, (44, 71)), ("strip_128x64_ks2", "strip_128x64_ks2")),
    ((4, 1, (8, 17)), ("strip_128x64_ks2", "strip_128x64_ks2")),
    ((4, 0, (50, 250)), ("r3_body_ks2", "r3_body_ks2")),
    ((4, 0, (87, 141)), ("h3_128x128_ks2", "h3_128x128_ks2")),
    ((2, 1, (8, 17)), ("strip_128x128", "strip_128x128")),
    ((2, 0, (50, 249)), ("r3_body", "r3_body")),
    ((1, 1, (8, 17)), ("strip_128x64", "strip_128x64")),
    # not in the issue's table: the one rule left that an input up to 2048 x 2048 reaches (layer1 at 32 x 32)
    ((1, 1, (7, 18)), ("h3_256x64", "h3_256x64")),
]
BATCH = 2  # frame 1 scaled by stage_cases.FACTORS[1]

# whole-model inputs (H, W) -> {layer: the rules of its four convs (block 0 conv1, conv2, block 1 conv1, conv2)}
MODEL_CASES = {
    (800, 800): {3: ("h3_128x128", "h3_128x128", "strip_64x128", "strip_64x128"),
                 4: ("h3_128x128_ks2", "h3_128x128_ks2", "strip_128x64_ks2", "strip_128x64_ks2")},
    (896, 896): {2: ("r3_body", "r3_body", "strip_128x128", "strip_128x128"),
                 3: ("r3_body", "r3_body", "strip_128x128", "strip_128x128"),
                 4: ("h3_128x128_ks2", "h3_128x128_ks2", "strip_128x64_ks2", "strip_128x64_ks2")},
    (1792, 1792): {4: ("r3_body_ks2", "r3_body_ks2", "strip_128x128_ks2", "strip_128x128_ks2")},
}
