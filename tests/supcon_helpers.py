"""Generated ROCO trees for the SupCon data-layer tests: the train table carries the three back-translation columns
(id, name, caption, fr, de, es) that pretrain/roco_supcon_train.py reads, plus rows named like the three the reference
removes (their images on disk, so only the name drop takes them out).  The validation split and vocabularies are
feeder_helpers.make_roco_tree's."""
import csv
import os

import numpy as np

from feeder_helpers import CAPTIONS, SIZES, make_roco_tree, write_jpeg
from test_augment import synth_image

DROPPED = ("PMC4345544_yjbm_88_1_93_g04.jpg", "PMC4240561_MA-68-291-g002.jpg", "PMC4093298_jadp-03-059-g02.jpg")


def translations(i):
    """the three translation cells of train row i: distinct sentences, so a test can tell the columns apart"""
    return (f"fr {CAPTIONS[(i + 1) % len(CAPTIONS)]}", f"de {CAPTIONS[(i + 4) % len(CAPTIONS)]}  ",
            f"es {CAPTIONS[(i + 6) % len(CAPTIONS)]}")


def make_supcon_tree(root, n_train=9, n_val=5, missing=(3, 5), short_row=None, empty_cell=None, seed=7):
    """train rows i < n_train are PMC{2000 + i}_train.jpg (no image for i in `missing`); the three DROPPED names go in
    after rows 0, 2 and 6.  short_row = i writes row i with 5 fields; empty_cell = (i, c) leaves column c of row i
    empty.  Returns (root, [(name, caption, (t3, t4, t5))] of the rows SupCon keeps, in file order)."""
    make_roco_tree(root, n_train=0, n_val=n_val, missing=(), seed=seed)
    rng = np.random.default_rng(seed)
    d = os.path.join(root, "train", "radiology")
    kept = []
    with open(os.path.join(d, "traindata.csv"), "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(["id", "name", "caption", "fr", "de", "es"])
        for i in range(n_train):
            name = f"PMC{2000 + i}_train.jpg"
            cap = CAPTIONS[(i * 3 + 1) % len(CAPTIONS)]
            row = [f"ROCO_{i:05d}", name, cap] + list(translations(i))
            if short_row == i:
                row = row[:5]
            if empty_cell is not None and empty_cell[0] == i:
                row[empty_cell[1]] = "  "
            w.writerow(row)
            if i not in missing:
                h, wd = SIZES[(i * 3) % len(SIZES)]
                write_jpeg(os.path.join(d, "images", name), synth_image(rng, h, wd))
                kept.append((name, cap.strip(), tuple(t.strip() for t in translations(i))))
            if i in (0, 2, 6):
                extra = DROPPED[(0, 2, 6).index(i)]
                w.writerow([f"ROCO_X{i}", extra, CAPTIONS[i % len(CAPTIONS)]] + list(translations(i + 1)))
                write_jpeg(os.path.join(d, "images", extra), synth_image(rng, 64, 80))
    return root, kept
