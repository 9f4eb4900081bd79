"""Generated on-disk trees for the data-layer tests: ROCO (<root>/<split>/radiology/<split>data.csv + images/) and
VQA-Med 2019 (traindf / valdf / testdf.csv + {Train,Val,Test}/images/), JPEGs made from test_augment.synth_image
arrays, a med_vocab.pkl, and the WordPiece vocabulary of tests/golden/text_vocab.txt.  Plus the CPU rebuild of a
device batch: PIL decode -> oracle.augment_oracle with the feeder's recorded params -> text.py with the same seeds."""
import csv
import os
import pickle

import numpy as np
import torch
from PIL import Image

from test_augment import synth_image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VOCAB = os.path.join(ROOT, "tests", "golden", "text_vocab.txt")
MED_VOCAB = {"organ": ["lung", "liver", "kidney", "heart"], "finding": ["mass", "lesion", "fracture", "effusion"]}

CAPTIONS = ["  Axial CT of the chest, showing a mass in the left upper lobe.  ",
            'MRI of the brain: "large" lesion, no edema',
            "chest x-ray with bilateral pleural effusion",
            "Coronal CT, liver and kidney, normal",
            "fracture of the left bone, arrow shows the lesion",
            "contrast enhanced scan of the abdomen; small cyst",
            "sagittal mri, 4 mm nodule in the right lung",
            "heart is normal, lungs are clear"]
QUESTIONS = [("what organ is shown in this image?", "Lung", "Organ"), ("which plane is this?", "Axial", "Plane"),
             ("is this normal?", "yes", "Binary"), ("what is the abnormality?", "Mass", "Abnormality"),
             ("which modality is shown?", "CT", "Modality"), ("where is the lesion?", "LIVER", "Organ")]
SIZES = [(224, 224), (100, 120), (300, 400), (257, 231), (37, 200), (200, 37), (150, 150), (500, 380)]


def write_jpeg(path, arr):
    Image.fromarray(arr).save(path, quality=92)


def make_roco_tree(root, n_train=18, n_val=6, missing=(3, 11), seed=0):
    """rows `missing` of the train table name images that are not on disk"""
    rng = np.random.default_rng(seed)
    for split, n, fname in (("train", n_train, "traindata.csv"), ("validation", n_val, "valdata.csv")):
        d = os.path.join(root, split, "radiology")
        os.makedirs(os.path.join(d, "images"))
        with open(os.path.join(d, fname), "w", newline="") as f:
            w = csv.writer(f)
            w.writerow(["id", "name", "caption"])
            for i in range(n):
                name = f"PMC{1000 + i}_{split}.jpg"
                w.writerow([f"ROCO_{i:05d}", name, CAPTIONS[(i * 3 + len(split)) % len(CAPTIONS)]])
                if split == "train" and i in missing:
                    continue
                h, wd = SIZES[(i + len(split)) % len(SIZES)]
                write_jpeg(os.path.join(d, "images", name), synth_image(rng, h, wd))
    os.makedirs(os.path.join(root, "vocab"))
    with open(os.path.join(root, "vocab", "med_vocab.pkl"), "wb") as f:
        pickle.dump(MED_VOCAB, f)
    return root


def make_vqa_tree(root, n=(10, 5, 7), seed=1):
    rng = np.random.default_rng(seed)
    for (split, folder, fname), cnt in zip((("train", "Train", "traindf.csv"), ("val", "Val", "valdf.csv"),
                                            ("test", "Test", "testdf.csv")), n):
        os.makedirs(os.path.join(root, folder, "images"))
        with open(os.path.join(root, fname), "w", newline="") as f:
            w = csv.writer(f)
            w.writerow(["img_id", "question", "answer", "category", "mode"])
            for i in range(cnt):
                img_id = f"synpic{split}{i}"
                q, a, c = QUESTIONS[(i + len(split)) % len(QUESTIONS)]
                w.writerow([img_id, q, a, c, split])
                h, wd = SIZES[(i * 5 + len(split)) % len(SIZES)]
                write_jpeg(os.path.join(root, folder, "images", img_id + ".jpg"), synth_image(rng, h, wd))
    return root


def tokenizer():
    from mmvqa_amd import text
    return text.BertWordPiece(VOCAB)


def rebuild_images(paths, params, size):
    """CPU rebuild of a device batch's images: (uint8 [B, S, S, 3], fp32 [B, 3, S, S])"""
    from oracle import augment_oracle as AO
    from mmvqa_amd import data as D
    u8, f = [], []
    for n, p in enumerate(paths):
        arr = D.decode(p)
        a, t = AO.train_transform(arr, params[n], size) if params is not None else AO.val_transform(arr, size)
        u8.append(torch.from_numpy(np.ascontiguousarray(a)))
        f.append(t)
    return torch.stack(u8), torch.stack(f)
