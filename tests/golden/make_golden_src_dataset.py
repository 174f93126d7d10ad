"""Fixture for the raw-file image-audio dataset (vipant_amd/data/image_audio.py): what the REFERENCE's own
`ImageAudioDatasetSrc._process_item` (cvap/data/image_audio.py:131-151) makes of a 7-record toy index in evaluation mode.

    python tests/golden/make_golden_src_dataset.py /path/to/reference      # writes tests/golden/src_dataset.json (data only)

The reference's image_audio.py is loaded by file path inside a stub package, with stub modules for the imports `_process_item` does not
need (torchaudio, tqdm, einops, its own `.audio` / `.image` subpackages).  The dataset object is made without its constructor (which
would build the transforms) and given the fields `_process_item` reads.  Recorded: the toy index and, for each spelling of the clip key
(`clip` / `aclip`) and `frame_emb` unset / set, the (name, clip file, frame file, frame embedding file) of every record and the frame
index the evaluation rule picked.  The data root is the literal `ROOT`.
"""
import importlib.util
import json
import os
import sys
import types

HERE = os.path.dirname(os.path.abspath(__file__))

RECORDS = [
    {"id": "a0", "dir": "", "clip": ["wav"], "frame": "png"},
    {"id": "a1", "dir": "sub", "clip": ["wav"], "frame": ["000.png"]},
    {"id": "a2", "dir": "", "clip": ["wav"], "frame": ["000.png", "001.png"]},
    {"id": "a3", "dir": "sub/deep", "clip": ["wav"], "frame": ["000.png", "001.png", "002.png", "003.png", "004.png"]},
    {"id": "a4", "dir": "", "clip": ["wav"], "frame": ["000.png", "001.png", "002.png", "003.png", "004.png", "005.png"]},
    {"id": "a5", "dir": "sub", "clip": ["flac", "wav"], "frame": "jpg"},
    {"id": "a6", "dir": "", "clip": ["wav"], "frame": ["000.v1.png", "001.v1.png"]},
]


def load_reference(root):
    def stub(name, **kw):
        m = types.ModuleType(name)
        m.__dict__.update(kw)
        sys.modules[name] = m
        return m

    class Anything:
        def __init__(self, *a, **k):
            pass
    for name in ("torchaudio", "tqdm", "einops"):
        stub(name, tqdm=Anything, rearrange=Anything, repeat=Anything)
    pkg = stub("reference_data")
    pkg.__path__ = []
    stub("reference_data.audio", make_transform=Anything, _extract_kaldi_spectrogram=Anything, FbankTransform=Anything)
    stub("reference_data.image", make_clip_image_transform=Anything, BarlowImageTransform=Anything)
    spec = importlib.util.spec_from_file_location("reference_data.image_audio", os.path.join(root, "cvap", "data", "image_audio.py"))
    mod = importlib.util.module_from_spec(spec)
    sys.modules["reference_data.image_audio"] = mod
    spec.loader.exec_module(mod)
    return mod


def main(root):
    ref = load_reference(root)
    cases = []
    for akey in ("clip", "aclip"):
        records = [{(akey if k == "clip" else k): v for k, v in r.items()} for r in RECORDS]
        for frame_emb in (None, "emb"):
            ds = object.__new__(ref.ImageAudioDatasetSrc)
            ds.dataset, ds.train = records, False
            ds.aclip_key = "clip" if "clip" in records[0] else "aclip"
            ds.frame_key = "frame"
            ds.cfg = types.SimpleNamespace(data_root="ROOT", frame_emb=frame_emb)
            items = []
            for i, r in enumerate(records):
                name, aclip_file, frame_file, frame_emb_file = ds._process_item(i)
                index = None if isinstance(r["frame"], str) else [f"ROOT/{r['dir'] + '/' if r['dir'] else ''}frame/{name}.{f}"
                                                                  for f in r["frame"]].index(frame_file)
                items.append({"name": name, "clip_file": aclip_file, "frame_file": frame_file, "frame_emb_file": frame_emb_file,
                              "frame_index": index})
            cases.append({"clip_key": akey, "frame_emb": frame_emb, "items": items})
    with open(os.path.join(HERE, "src_dataset.json"), "w") as f:
        json.dump({"records": RECORDS, "cases": cases}, f, indent=1)
        f.write("\n")
    print(f"wrote {len(cases)} cases x {len(RECORDS)} records")


if __name__ == "__main__":
    main(sys.argv[1])
