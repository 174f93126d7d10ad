"""Fixture for the classification datasets (vipant_amd/data/classify.py): what the REFERENCE's own x-fold builders
(cvap/data/esc50.py:224-324), `build_audioset_label_map` / `build_filter_set` (cvap/data/audioset_hub.py:32-106) and `AudiosetSrc`
(cvap/data/audioset_cls.py:193-310: index reading, `sample_weights`, `_process_item` on the clf path) make of toy inputs.

    python tests/golden/make_golden_clf_dataset.py /path/to/reference      # writes tests/golden/clf_dataset.json (data only)

The reference's modules are loaded by file path: its `clip` package as it is (stub `ftfy` = identity), esc50.py, audioset_cls.py and
audioset_hub.py inside a stub package with stub modules for the imports the recorded functions do not need (`tabulate` / `termcolor`
among them: the label table is printed and thrown away).  The toy files are written into a temporary directory; every recorded path
has it replaced by the literal `ROOT`.  Recorded, with the inputs (file texts) they were made from:
  esc50 / us8k   the meta CSV, the `meta/ensemble.json` prompt file, and per prompt (`the sound of`, empty, `ensemble`): the
                 (train, eval) lists of every fold, lid2str, lid2int (token rows, zero padded) and label_map;
  audioset       a toy ontology of 8 classes of which 5 occur in the FIRST row of a clip of the toy segments CSV; the label map
                 without and with a prompt; the three filter-set forms and three broken ones (-> None);
  tagging        an index of 6 records per clip-key spelling (with and without `dir`, duplicate labels): `_process_item` of every
                 record (name, multi-hot row, clip file), `sample_weights`, and the ids the index reading keeps under a filter set
                 and under `eval_samples`.
The script tokenises every prompt with the reference's tokenizer over its WHOLE vocabulary file and with the repository's tokenizer
over the committed head (bpe_simple_vocab_16e6.head.txt.gz) and refuses to write unless the ids agree.
"""
import importlib.util
import io
import json
import os
import sys
import tempfile
import types
from contextlib import redirect_stdout

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

ESC_CLASSES = ["dog", "rain", "sea_waves", "crow", "clock_tick"]
ESC_META = "filename,fold,target,category,esc10,src_file,take\n" + "".join(
    f"{fold}-{1000 + 7 * k}-A-{(k * 3 + fold) % 5}.wav,{fold},{(k * 3 + fold) % 5},{ESC_CLASSES[(k * 3 + fold) % 5]},"
    f"{'True' if k else 'False'},{1000 + 7 * k},A\n" for k in range(2) for fold in (3, 1, 5, 2, 4))
US_CLASSES = ["air_conditioner", "car_horn", "dog_bark", "siren"]
US_META = "slice_file_name,fsID,start,end,salience,fold,classID,class\n" + "".join(
    f"{2000 + k}-{(k + fold) % 4}-0-{k}.wav,{2000 + k},0.5,4.5,{1 + k % 2},{fold},{(k + fold) % 4},{US_CLASSES[(k + fold) % 4]}\n"
    for k in range(2) for fold in (10, 2, 7, 1, 4, 9, 3, 8, 6, 5))
ENSEMBLE = {
    "dog": ["a photo of a dog", "a dog barks", "the bark of a dog", "a photo of the dog", "never read"],
    "rain": ["a photo of rain", "rain falls", "heavy rain on a roof", "water drops"],
    "sea waves": ["a photo of sea waves", "waves on the sea", "the sea", "water and wind", "never read", "nor this"],
    "crow": ["a photo of a crow", "a crow calls", "birds", "a bird sings"],
    "clock tick": ["a photo of a clock", "a clock ticks", "the tick of a clock", "not a photo of time"],
    "air conditioner": ["unused"], "car horn": ["unused"], "dog bark": ["unused"], "siren": ["unused"],
}
PROMPTS = ["the sound of", "", "ensemble"]

ONTOLOGY = [{"id": f"/m/0{c}", "name": name, "description": "", "child_ids": []} for c, name in zip(
    "abcdefgh", ["Speech", "Dog", "Rain on Surface", "Engine", "Bird", "Water", "Wind", "Music"])]
SEGMENTS = ("# Segments csv created Sun Mar  5 10:54:25 2017\n# num_ytids=6, num_segs=7, num_unique_labels=6, num_positive_labels=11\n"
            "# YTID, start_seconds, end_seconds, positive_labels\n"
            'y0, 0.000, 10.000, "/m/0a,/m/0b"\n'
            'y1, 30.000, 40.000, "/m/0c"\n'
            'y2, 5.000, 15.000, "/m/0e,/m/0a"\n'
            'y1, 50.000, 60.000, "/m/0d"\n'                      # a second row of y1: not read for the class set
            'y3, 0.000, 9.000, "/m/0h"\n'
            'y4, 12.000, 22.000, "/m/0b,/m/0c,/m/0e"\n'
            'y5, 1.000, 11.000, "/m/0h,/m/0a"\n')
FILTER_FILES = {
    "keep.csv": "y0\ny2\n  y5  \n",
    "per_label.10k": json.dumps({"/m/0a": ["y0", "y2"], "/m/0b": ["y4", "y0"], "/m/0h": []}),
    "neighbours.json": "".join(json.dumps(row) + "\n" for row in (
        {"y0": [["y1", 0.9], ["y2", 0.8], ["y3", 0.7]]}, {"y5": [["y4", 0.5]]})),
}
FILTER_SETS = ["keep.csv,0", "per_label.10k,0", "neighbours.json,2", "neighbours.json,1", "missing.csv,1", "keep.csv", None,
               "neighbours.json,two"]
TAG_RECORDS = [
    {"id": "y0", "dir": "", "clip": ["wav"], "frame": "png", "labels": ["/m/0a", "/m/0b"]},
    {"id": "y1", "dir": "bal", "clip": ["wav"], "frame": "png", "labels": ["/m/0c"]},
    {"id": "y2", "dir": "", "clip": ["wav", "flac"], "frame": "png", "labels": ["/m/0e", "/m/0a", "/m/0e"]},      # a duplicate label
    {"id": "y3", "dir": "unbal/part1", "clip": ["wav"], "frame": "png", "labels": ["/m/0h"]},
    {"id": "y4", "dir": "bal", "clip": ["wav"], "frame": "png", "labels": ["/m/0b", "/m/0c", "/m/0e"]},
    {"id": "y5", "dir": "", "clip": ["wav"], "frame": "png", "labels": ["/m/0h", "/m/0a", "/m/0h", "/m/0a"]},
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
    stub("reference_data.audio", make_transform=lambda *a, **k: (None, None), _extract_kaldi_spectrogram=Anything, RandomCrop=Anything)
    stub("reference_data.image", make_clip_image_transform=Anything)
    stub("reference_data.audiocaps", AudioCapDatasetSrc=Anything)
    stub("reference_data.audioset_clf", AudiosetDatasetNpz=Anything, ImageAudioCollator=Anything)
    data = os.path.join(root, "cvap", "data")
    return (sys.modules["clip"], load("reference_data.esc50", os.path.join(data, "esc50.py")),
            load("reference_data.audioset_cls", os.path.join(data, "audioset_cls.py")),
            load("reference_data.audioset_hub", os.path.join(data, "audioset_hub.py")))


def write(path, text):
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        f.write(text)


def fold_lists(loader_tuple):
    """The lists the lazy loader factories were closed over (their default argument): nothing is built."""
    return [{"train": fn_train.__defaults__[0], "eval": fn_eval.__defaults__[0]} for fn_train, fn_eval in loader_tuple]


def same_ids_with_the_head(clip, texts):
    from vipant_amd.tokenizer import SimpleTokenizer, tokenize
    head = SimpleTokenizer(os.path.join(HERE, "bpe_simple_vocab_16e6.head.txt.gz"))
    assert tokenize(texts, as_list=True, tokenizer=head) == clip.tokenize(texts, as_list=True), "the head vocabulary tokenises differently"


def main(root):
    clip, esc50, audioset_cls, audioset_hub = load_reference(root)
    out = {"esc50": {"meta": ESC_META, "ensemble": ENSEMBLE, "cases": []}, "us8k": {"meta": US_META, "ensemble": ENSEMBLE, "cases": []}}
    texts = []
    with tempfile.TemporaryDirectory() as tmp:
        write(f"{tmp}/esc/meta/esc50.csv", ESC_META)
        write(f"{tmp}/esc/meta/ensemble.json", json.dumps(ENSEMBLE))
        write(f"{tmp}/us/metadata/UrbanSound8K.csv", US_META)
        write(f"{tmp}/us/meta/ensemble.json", json.dumps(ENSEMBLE))
        for key, sub, name, build in (("esc50", "esc", "esc50", esc50.build_dataloader_list_esc50),
                                      ("us8k", "us", "UrbanSound8K", esc50.build_dataloader_list_us8k)):
            for prompt in PROMPTS:
                cfg = types.SimpleNamespace(running=types.SimpleNamespace(data_root=f"{tmp}/{sub}", data_name=name, prompt=prompt))
                shown = io.StringIO()
                with redirect_stdout(shown):
                    loader_tuple, lid2str, lid2int, label_map = build(cfg)
                strings = eval(shown.getvalue().strip().splitlines()[-1])          # the reference prints the prompt strings
                texts += strings
                out[key]["cases"].append({
                    "prompt": prompt, "folds": fold_lists(loader_tuple), "lid2str": {str(k): v for k, v in lid2str.items()},
                    "prompts": strings, "lid2int": lid2int.tolist(),
                    "label_map": None if label_map is None else {str(k): v for k, v in label_map.items()}})

        aroot = f"{tmp}/as"
        write(f"{aroot}/ontology.json", json.dumps(ONTOLOGY))
        write(f"{aroot}/eval_segments.csv", SEGMENTS)
        for fname, text in FILTER_FILES.items():
            write(f"{aroot}/{fname}", text)
        maps = []
        for prompt in ("", " the sound of "):
            lm = audioset_hub.build_audioset_label_map(aroot, label_map="ontology,eval_segments", prompt=prompt)
            texts += [v[1] for v in lm.values()]
            maps.append({"prompt": prompt, "label_map": {k: list(v) for k, v in lm.items()}})
        filters = []
        for fs in FILTER_SETS:
            got = audioset_hub.build_filter_set(aroot, fs)
            filters.append({"filter_set": fs, "samples": None if got is None else sorted(got)})
        out["audioset"] = {"ontology": ONTOLOGY, "segments": SEGMENTS, "filter_files": FILTER_FILES, "label_maps": maps, "filters": filters}

        label_map = {k: tuple(v) for k, v in maps[1]["label_map"].items()}
        tagging = []
        for akey in ("clip", "aclip"):
            records = [{(akey if k == "clip" else k): v for k, v in r.items()} for r in TAG_RECORDS]
            write(f"{aroot}/src_{akey}.csv", "".join(json.dumps(r) + "\n" for r in records))

            def dataset(train, weighted, filter_set=None, eval_samples=250000):
                cfg = types.SimpleNamespace(
                    data_root=aroot, cat_label=False, eval_samples=eval_samples, prompt="the sound of", frame_key="frame", resolution=224,
                    imagine=False, clf=True, frame_emb=None, text_emb=None,
                    audio=types.SimpleNamespace(norms=[-4.9, 5.7], num_mel_bins=64))
                with redirect_stdout(io.StringIO()):
                    return audioset_cls.AudiosetSrc(cfg, f"src_{akey}", train, label_map, weighted, filter_set=filter_set)
            ds = dataset(True, True)
            items = []
            for i in range(len(records)):
                item, label, aclip_file, frame_file, frame_emb_file = ds._process_item(i)
                assert frame_file is None and frame_emb_file is None and item["text"] == [0]
                items.append({"name": item["name"], "label": label, "clip_file": aclip_file.replace(aroot, "ROOT")})
            reads = []
            for train, weighted, fs, es in ((True, True, ["y0", "y2", "y4", "y5"], 250000), (False, False, None, 3),
                                            (False, True, None, 4), (False, False, ["y1", "y3", "y4", "y5"], 4)):
                d = dataset(train, weighted, None if fs is None else set(fs), es)
                reads.append({"train": train, "weighted": weighted, "filter_set": fs, "eval_samples": es,
                              "ids": [r["id"] for r in d.dataset],
                              "sample_weights": d.sample_weights.tolist() if weighted else None})
            tagging.append({"clip_key": akey, "records": records, "items": items, "sample_weights": ds.sample_weights.tolist(),
                            "reads": reads})
        out["tagging"] = {"label_map_prompt": maps[1]["prompt"], "cases": tagging}
    same_ids_with_the_head(clip, sorted(set(texts)))
    with open(os.path.join(HERE, "clf_dataset.json"), "w") as f:
        json.dump(out, f, indent=None, separators=(",", ":"))
        f.write("\n")
    print(f"wrote clf_dataset.json: {len(out['esc50']['cases'])} + {len(out['us8k']['cases'])} x-fold cases, "
          f"{len(maps[0]['label_map'])} of {len(ONTOLOGY)} classes, {len(filters)} filter sets, {len(tagging)} tagging cases; "
          f"{len(set(texts))} prompt strings agree between the whole vocabulary and the head")


if __name__ == "__main__":
    main(sys.argv[1])
