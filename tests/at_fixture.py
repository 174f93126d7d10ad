"""Directories in the layout of the reference's caption datasets, generated into a temporary path with the writers of
tests/src_fixture.py: an AudioCaps index (`{name}.csv`, one JSON record per line with `captions`; clips under `{dir/}clip/`, PNG frames
under `{dir/}frame/` when asked for) and a Clotho fold (`clotho_{fold}.csv` with file_name, caption_1 .. caption_5; clips inside
`{fold}/` under their file names).  Shared by tests/test_audio_text_cpu.py and tests/test_at_trainer_gpu.py."""
import csv
import json
import os

import numpy as np

import src_fixture as SF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BPE = os.path.join(ROOT, "tests", "golden", "bpe_simple_vocab_16e6.head.txt.gz")

# 8 x 5 captions of 6 to 40 tokens (SOT and EOT counted); a clip's captions differ in length, so batches differ in width.  Every
# word is one token of the CLIP vocabulary.
WORDS = ("a man speaks while a dog runs in the background and then rain falls on a tin roof as an engine flows nearby "
         "before birds sing and water pours into a glass while wind blows over the hill far away").split()


def captions_for(i, count=5):
    """`count` captions of clip i, of 4 to 38 words (one token each) -> 6 to 40 tokens with SOT and EOT; the longest caption of the
    clips 0 .. 3 has 40 tokens, that of the clips 4 .. 7 has 35: two evaluation batches of four differ in width."""
    out = []
    for k in range(count):
        n = (4, 12, 21, 30, 38)[(k + i) % 5] - (i % 3 if (k + i) % 5 else 0)
        n = min(n, 26 + i) if i >= 4 else n
        out.append(" ".join(WORDS[(7 * (5 * i + k) + j) % len(WORDS)] for j in range(n)))      # 40 words, 40 different heads
    return out


def write_index(root, name, records):
    with open(f"{root}/{name}.csv", "w") as f:
        for r in records:
            f.write(json.dumps(r) + "\n")


def make_audiocaps_dir(root, name, seconds, channels, ncaptions=None, sub_dirs=None, frame_hw=None, nframes_per_item=None, seed=5,
                       rate=SF.SR, clip_key="clip"):
    """Writes len(seconds) clips and `{root}/{name}.csv` -> (records, clips int16 [n, ch], frames: lists of uint8 [h, w, 3])."""
    g = np.random.default_rng(seed)
    records, clips, frames = [], [], []
    for i, (sec, ch) in enumerate(zip(seconds, channels)):
        ident = f"y{i}"
        sub = sub_dirs[i] if sub_dirs else ""
        base = f"{root}/{sub + '/' if sub else ''}"
        pcm = SF.noise_clip(g, int(round(sec * rate)), ch, amp=800 + 1100 * i)       # clips differ in level: distinct features
        SF.write_wav(f"{base}{clip_key}/{ident}.wav", pcm, rate=rate)
        k = nframes_per_item[i] if nframes_per_item else 0
        names = "png" if k == 0 else [f"{j:03d}.png" for j in range(k)]
        mine = []
        if frame_hw is not None:
            for fname in ([names] if k == 0 else names):
                fr = g.integers(0, 256, size=(frame_hw[i][0], frame_hw[i][1], 3), dtype=np.int64).astype(np.uint8)
                SF.write_png(f"{base}frame/{ident}.{fname}", fr)
                mine.append(fr)
        records.append({"id": ident, "dir": sub, clip_key: ["wav"], "frame": names, "labels": [f"/m/{i % 3}"],
                        "captions": captions_for(i, ncaptions[i] if ncaptions else 5)})
        clips.append(pcm)
        frames.append(mine)
    write_index(root, name, records)
    return records, clips, frames


def make_clotho_dir(root, fold, seconds, rate=44100, seed=9, channels=None):
    """Writes `{root}/clotho_{fold}.csv` and its clips `{root}/{fold}/{file_name}` -> (rows, clips)."""
    g = np.random.default_rng(seed)
    rows, clips = [], []
    for i, sec in enumerate(seconds):
        fname = f"clip {i:02d} - take.wav"
        pcm = SF.noise_clip(g, int(round(sec * rate)), channels[i] if channels else 1, amp=1500 + 1700 * i)
        SF.write_wav(f"{root}/{fold}/{fname}", pcm, rate=rate)
        row = {"file_name": fname}
        row.update({f"caption_{k + 1}": c for k, c in enumerate(captions_for(i))})
        rows.append(row)
        clips.append(pcm)
    with open(f"{root}/clotho_{fold}.csv", "w", newline="") as f:
        w = csv.DictWriter(f, fieldnames=["file_name"] + [f"caption_{k}" for k in range(1, 6)])
        w.writeheader()
        w.writerows(rows)
    return rows, clips
