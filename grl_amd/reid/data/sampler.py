"""The reference's pair sampler for MARS / DukeMTMC-VideoReID (reid/data/sampler.py:83-125), restated."""
from collections import defaultdict

import numpy as np
import torch
from torch.utils.data import Sampler


class RandomPairSamplerForMars(Sampler):
    """Every tracklet once per epoch in ``torch.randperm`` order, each followed by a positive of the same pid: one drawn
    uniformly from the pid's tracklets of ANOTHER camera; for a pid seen by one camera, from its other tracklets; for a
    pid with a single tracklet, the tracklet itself.  ``2 * len(data_source)`` indices.

    The random calls are the reference's, in its order -- one ``torch.randperm(n)``, then one ``np.random.choice`` over
    the candidates of every anchor that has any -- so a seeded run draws the reference's index sequence."""

    def __init__(self, data_source):
        self.data_source = data_source
        self.num_samples = len(data_source)
        pid_index, pid_cam = defaultdict(list), defaultdict(list)
        for index, (_, pid, cam) in enumerate(data_source):
            pid_index[pid].append(index)
            pid_cam[pid].append(cam)
        # per tracklet: the pid's tracklet list and the positions in it a positive may come from (None: itself)
        self._cands = []
        for index, (_, pid, cam) in enumerate(data_source):
            idx, cams = pid_index[pid], pid_cam[pid]
            if len(set(cams)) > 1:
                pos = [k for k, c in enumerate(cams) if c != cam]
            elif len(idx) > 1:
                pos = [k for k, j in enumerate(idx) if j != index]
            else:
                pos = None
            self._cands.append((idx, pos))

    def __len__(self):
        return self.num_samples * 2

    def __iter__(self):
        ret = []
        for i in torch.randperm(self.num_samples).tolist():
            idx, pos = self._cands[i]
            ret.append(i)
            ret.append(idx[0] if pos is None else idx[pos[np.random.choice(len(pos))]])
        return iter(ret)
