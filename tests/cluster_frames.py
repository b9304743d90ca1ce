"""Frames for the cluster tests: a few hundred rows built from a few dozen base strings with 0 .. 2 edits each -- so that clusters
of several members exist and chain (a ~ b ~ c with a and c two edits either side of b) -- plus empty strings, strings longer than
32 bytes and non-ASCII strings, whose pairs go through the join's slow fallback and contribute edges too."""
import random

import gen

# per measure: the cutoff at which the frame below holds clusters that chain without collapsing into one (chosen on the CPU model;
# every GPU test first asserts on the model that the frame is worth it)
MIN_SCORE = {"levenshtein": 0.8, "jaro": 0.9, "jaro_winkler": 0.92, "jaccard": 0.8, "sorensen_dice": 0.9, "ratio": 0.88, "token_sort_ratio": 0.88}


def frame(seed, rows=150, bases=20):
    rng = random.Random(seed)
    base = [gen.rand_string(rng, gen.ASCII_LOWER, 4, 9) + " " + gen.rand_string(rng, gen.ASCII_LOWER, 5, 10) for _ in range(bases)]
    base += [gen.rand_string(rng, gen.ASCII_LOWER, 12, 16) + " " + gen.rand_string(rng, gen.ASCII_LOWER, 20, 24) for _ in range(4)]  # > 32 bytes
    base += [gen.rand_string(rng, "abcdeéüñ日本", 8, 12) + "é" for _ in range(4)]                                                      # non-ASCII
    out = []
    for _ in range(rows):
        b = rng.choice(base)
        out.append(gen.edit(rng, b, gen.ASCII_LOWER, rng.randint(0, 2)))
    out += [""] * 3
    rng.shuffle(out)
    return out
