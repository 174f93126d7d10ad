"""Dataset builders (cvap/data): host-only code that loader workers run.  Nothing in this package imports the HIP binding or touches
torch.cuda; the decoded bytes it yields become tensors on the device in the trainers' `make_batch`."""
from .audio_text import (AudioCapSrc, AudioTextSrc, CaptionCollator, build_audio_text_dataloader,  # noqa: F401
                         build_audiocaps_data_list, build_clotho_data_list, collate_text)
from .classify import (AudiosetSrc, TaggingCollator, TaggingLabels, XFoldCollator, XFoldSrc,  # noqa: F401
                       build_audioset_clf_dataloader, build_audioset_label_map, build_filter_set, build_xfold_dataloader,
                       build_xfold_dataloader_list)
from .decode import read_frame, read_wav  # noqa: F401
from .image_audio import (FrameBatch, ImageAudioSiameseSrc, ImageAudioSrc, PcmBatch, SecondView,  # noqa: F401
                          SiameseSrcCollator, SrcCollator, build_image_audio_dataloader)

__all__ = ["read_wav", "read_frame", "FrameBatch", "PcmBatch", "SecondView", "ImageAudioSrc", "ImageAudioSiameseSrc", "SrcCollator",
           "SiameseSrcCollator", "build_image_audio_dataloader", "AudioCapSrc", "AudioTextSrc", "CaptionCollator", "collate_text",
           "build_clotho_data_list", "build_audiocaps_data_list", "build_audio_text_dataloader", "XFoldSrc", "XFoldCollator",
           "build_xfold_dataloader", "build_xfold_dataloader_list", "build_audioset_label_map", "build_filter_set", "AudiosetSrc",
           "TaggingLabels", "TaggingCollator", "build_audioset_clf_dataloader"]
