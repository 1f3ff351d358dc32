"""Tracklet indexes of the video re-id datasets (the reference's ``reid.dataset``, which its loaders reach through
``get_sequence``).  Parsing is host work done once per run, outside the hot path: what it yields -- lists of
(img_paths, pid, camid) -- feeds ``reid.data.RawVideoDataset``, whose frames are decoded and augmented on the device.

Unlike the reference, the indexes are rebuilt on every construction and nothing is written into the dataset root
(the reference caches ``split_*.json`` there; dataset mounts are often read-only, and a cache left by another root or
another ``min_seq_len`` would be silently reused).  Parsing MARS takes a few seconds."""
from .duke import DukeMTMCVidReID
from .mars import Mars

__all__ = ['Mars', 'DukeMTMCVidReID', 'get_sequence']

_FACTORY = {
    'mars': Mars,
    'duke': DukeMTMCVidReID,
}

_OPTICAL_FLOW = ('ilidsvidsequence', 'prid2011sequence')


def get_sequence(name, *args, **kwargs):
    """``get_sequence('mars' | 'duke', min_seq_len=0, root=None, data_dir=None, verbose=True)``."""
    if name in _OPTICAL_FLOW:
        raise NotImplementedError(
            "dataset '%s': the reference's loaders for it yield (image, optical flow, pid, camid) tuples, which its "
            "own GRL trainer (SEQTrainer) does not consume; only 'mars' and 'duke' are provided" % name)
    if name not in _FACTORY:
        raise KeyError("Unknown dataset", name)
    return _FACTORY[name](*args, **kwargs)
