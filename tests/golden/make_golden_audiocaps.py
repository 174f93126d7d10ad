"""Fixture for the caption datasets (vipant_amd/data/audio_text.py): what the REFERENCE's own `AudioCapDatasetSrc._process_item`
(cvap/data/audiocaps.py:81-115), text collator (cvap/data/audioset_clf.py:122-152 `ImageAudioCollator`) and
`build_clotho_data_list` (cvap/data/audio_text.py:169-194) make of toy inputs.

    python tests/golden/make_golden_audiocaps.py /path/to/reference      # writes tests/golden/audiocaps_dataset.json (data only)

The reference's modules are loaded by file path: its `clip` package as it is (with stub `ftfy` = identity, `torchvision`, `tqdm`),
audiocaps.py, audioset_clf.py and audio_text.py inside a stub package with stub modules for the imports the recorded functions do not
need.  The dataset objects are made without their constructors (which would build transforms) and given the fields `_process_item`
reads.  The data root is the literal `ROOT`.  Recorded:
  records   the toy index (6 records: with and without `dir`, frame as a string and as lists of 1, 2 and 5, 1 and 5 captions);
  cases     per clip-key spelling (`clip` / `aclip`) and (imagine, frame_emb) in (False, None), (True, None), (True, "emb"): name,
            text (all captions, tokenised), clip file, frame file and frame embedding file of every record in evaluation mode;
  collated  the text array of the reference's collator for a training-shaped batch (caption `pick[i]` of record i) and for an
            evaluation-shaped batch (all captions of the records `eval_records`), with zeros as dummy image / audio;
  clotho    a 3-row CSV and its data list without and with a prompt.
"""
import importlib.util
import json
import os
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))

FIVE = ["000.png", "001.png", "002.png", "003.png", "004.png"]
RECORDS = [
    {"id": "k0", "dir": "", "clip": ["wav"], "frame": "png", "labels": ["/m/0"],
     "captions": ["A man speaks while a dog barks in the background", "a dog barking", "Someone is talking and a dog's barking loudly",
                  "speech, then barks", "A man talks over a barking dog and the wind blows into the microphone the whole time"]},
    {"id": "k1", "dir": "train", "clip": ["wav"], "frame": ["000.png"], "labels": ["/m/1"], "captions": ["Rain falls on a tin roof"]},
    {"id": "k2", "dir": "", "clip": ["wav"], "frame": ["000.png", "001.png"], "labels": ["/m/2"],
     "captions": ["An engine idles", "an engine idling then revving", "A car's engine runs", "vroom vroom", "Engine noise at 3000 rpm"]},
    {"id": "k3", "dir": "train/deep", "clip": ["flac", "wav"], "frame": FIVE, "labels": ["/m/0", "/m/2"],
     "captions": ["Birds chirp & a rooster crows", "birds", "A rooster crowing, birds singing", "Chirping birds in the morning",
                  "wind and birds"]},
    {"id": "k4", "dir": "", "clip": ["wav"], "frame": "jpg", "labels": [], "captions": ["a duck quacks"]},
    {"id": "k5", "dir": "val", "clip": ["wav"], "frame": FIVE, "labels": ["/m/1"],
     "captions": ["Water pours into a glass", "water running", "Liquid being poured, it's splashing", "a tap runs",
                  "Someone fills a cup with water then stops"]},
]
CLOTHO_CSV = ("file_name,caption_1,caption_2,caption_3,caption_4,caption_5\n"
              "Distorted AM Radio noise.wav,A muddled noise of broken channel of the TV,A television blares the rhythm of a static TV.,"
              "Loud television static dips in and out of focus,The loud buzz of static constantly changes pitch and volume.,"
              "heavy static and the beginnings of a signal on a transistor radio\n"
              "rain_01.wav,\"Rain falls, steadily\",rain,It's raining,Heavy rain on a roof,water drops\n"
              "07 storm - orage.wav,A storm,Thunder rolls in the distance,a thunderstorm,\"wind, rain and thunder\",Storm sounds\n")


def load_reference(root):
    def stub(name, **kw):
        m = types.ModuleType(name)
        m.__dict__.update(kw)
        sys.modules[name] = m
        return m

    class Anything:
        def __init__(self, *a, **k):
            pass

    def load(name, path, **kw):
        spec = importlib.util.spec_from_file_location(name, path, **kw)
        mod = importlib.util.module_from_spec(spec)
        sys.modules[name] = mod
        spec.loader.exec_module(mod)
        return mod
    stub("ftfy", fix_text=lambda text: text)
    for name in ("torchaudio", "tqdm", "einops", "tabulate", "termcolor"):
        stub(name, tqdm=Anything, rearrange=Anything, repeat=Anything, tabulate=Anything, colored=Anything)
    tv = stub("torchvision")
    tv.transforms = stub("torchvision.transforms", **{k: Anything for k in ("InterpolationMode", "Compose", "Resize", "CenterCrop",
                                                                             "ToTensor", "Normalize")})
    load("clip", os.path.join(root, "clip", "__init__.py"), submodule_search_locations=[os.path.join(root, "clip")])
    pkg = stub("reference_data")
    pkg.__path__ = []
    stub("reference_data.audio", make_transform=Anything, _extract_kaldi_spectrogram=Anything)
    stub("reference_data.image", make_clip_image_transform=Anything)
    stub("reference_data.audioset_cls", print_label_dist=Anything, AudiosetNpz=Anything, AudiosetSrc=Anything)
    data = os.path.join(root, "cvap", "data")
    return (sys.modules["clip"], load("reference_data.audiocaps", os.path.join(data, "audiocaps.py")),
            load("reference_data.audioset_clf", os.path.join(data, "audioset_clf.py")),
            load("reference_data.audio_text", os.path.join(data, "audio_text.py")))


def main(root):
    clip, audiocaps, audioset_clf, audio_text = load_reference(root)
    cases = []
    for akey in ("clip", "aclip"):
        records = [{(akey if k == "clip" else k): v for k, v in r.items()} for r in RECORDS]
        for record in records:
            record["captions_bpe"] = clip.tokenize(record["captions"], as_list=True)
        for imagine, frame_emb in ((False, None), (True, None), (True, "emb")):
            ds = object.__new__(audiocaps.AudioCapDatasetSrc)
            ds.dataset, ds.train, ds.length, ds.rnd_cap = records, False, len(records), False
            ds.aclip_key = "clip" if "clip" in records[0] else "aclip"
            ds.frame_key = "frame"
            ds.cfg = types.SimpleNamespace(data_root="ROOT", frame_emb=frame_emb, imagine=imagine)
            items = []
            for i in range(len(records)):
                item, label, aclip_file, frame_file, frame_emb_file = ds._process_item(i)
                items.append({"name": item["name"], "text": item["text"], "clip_file": aclip_file, "frame_file": frame_file,
                              "frame_emb_file": frame_emb_file})
            cases.append({"clip_key": akey, "imagine": imagine, "frame_emb": frame_emb, "items": items})
    bpe = [clip.tokenize(r["captions"], as_list=True) for r in RECORDS]
    collate = audioset_clf.ImageAudioCollator()
    dummy = {"image": np.zeros((1, 1, 1, 1)), "audio": np.zeros((1, 2, 2)), "label": [0]}
    pick = [4, 0, 3, 1, 0, 2]
    train = collate([dict(dummy, text=bpe[i][p], name=RECORDS[i]["id"]) for i, p in enumerate(pick)])
    eval_records = [0, 2, 3, 5]
    evaln = collate([dict(dummy, text=bpe[i], name=RECORDS[i]["id"]) for i in eval_records])
    collated = {"train": {"pick": pick, "text": train[2].tolist(), "names": list(train[4])},
                "eval": {"eval_records": eval_records, "text": evaln[2].tolist(), "names": list(evaln[4])}}
    clotho = {"csv": CLOTHO_CSV, "lists": []}
    with tempfile.TemporaryDirectory() as tmp:
        with open(os.path.join(tmp, "clotho_development.csv"), "w") as f:
            f.write(CLOTHO_CSV)
        for prompt in ("", " the sound of  "):
            cfg = types.SimpleNamespace(data_root=tmp, prompt=prompt)
            clotho["lists"].append({"prompt": prompt, "data_name": "clotho_development",
                                    "records": audio_text.build_clotho_data_list(cfg, "clotho_development")})
    with open(os.path.join(HERE, "audiocaps_dataset.json"), "w") as f:
        json.dump({"records": RECORDS, "cases": cases, "collated": collated, "clotho": clotho}, f, indent=None, separators=(",", ":"))
        f.write("\n")
    print(f"wrote {len(cases)} cases x {len(RECORDS)} records; train text {np.shape(train[2])}, eval text {np.shape(evaln[2])}")


if __name__ == "__main__":
    main(sys.argv[1])
