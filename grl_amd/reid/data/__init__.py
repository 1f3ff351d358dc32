"""Input pipeline of the reference (reid/data): ``get_data`` keeps the reference's signature and return tuple
(dataloader.py:47-81).  'mars' and 'duke' index the dataset on the host (``reid.dataset``) and hand the frames to the
device: loader workers only read the JPEG files, engine.DevicePrefetcher decodes them on the GPU and SEQTrainer applies
the reference's RectScale / flip / erase / Normalize chain there (``GRL_DECODE=host``: Pillow decodes in the workers
instead).  'synthetic' serves synthetic MARS-shaped clips arranged as (anchor, positive) pairs -- the invariant
``Siamese.forward`` relies on (sampler.py:104-123)."""
import os

import torch
from torch.utils.data import DataLoader, Dataset

from grl_amd.synthetic import synth_clips

from .sampler import RandomPairSamplerForMars  # noqa: F401  (reid.data exports it, as upstream)


class SyntheticPairs(Dataset):
    """`n_pairs` x 2 clips; both clips of a pair share the pid, cameras differ."""

    def __init__(self, n_pairs, seq_len, num_classes=625, seed=0, raw=False, augment=False):
        self.n, self.t, self.k, self.seed = 2 * n_pairs, seq_len, num_classes, seed
        self.raw = raw or augment   # uint8 pixels (normalised on the device) instead of float32
        self.augment = augment      # also yield the flip / erase decisions: the device applies them

    def __len__(self):
        return self.n

    def __getitem__(self, i):
        clip = synth_clips(1, self.t, seed=self.seed * 100003 + i, raw=self.raw)[0]
        item = (clip, (i // 2 * 7919 + self.seed) % self.k, i % 2)
        if self.augment:
            from .augment import draw_clip_params
            item += (torch.tensor(draw_clip_params(self.t, clip.shape[-2], clip.shape[-1]), dtype=torch.int32),)
        return item


def get_data(dataset_name, split_id, data_dir, batch_size, seq_len, seq_srd, workers, only_eval=False):
    """-> (dataset, num_classes, train_loader, query_loader, gallery_loader), as the reference's get_data."""
    if dataset_name in ('mars', 'duke'):
        return _video_data(dataset_name, data_dir, batch_size, seq_len, workers, only_eval)
    if dataset_name != 'synthetic':
        if dataset_name in ('ilidsvidsequence', 'prid2011sequence'):
            raise NotImplementedError(
                "dataset '%s': the reference's loaders for it yield (image, optical flow, pid, camid) 4-tuples, which "
                "its own GRL trainer does not consume; use 'mars', 'duke' or 'synthetic'" % dataset_name)
        raise NotImplementedError(
            "dataset '%s': use 'mars', 'duke' or 'synthetic', or feed SEQTrainer/ATTEvaluator any loader that yields "
            "(imgs[B,T,3,256,128], pids, camids)" % dataset_name)
    train = SyntheticPairs(8 * batch_size, seq_len)
    loader = DataLoader(train, batch_size=batch_size, shuffle=False, drop_last=True, num_workers=0)
    q = DataLoader(SyntheticPairs(15, seq_len, seed=1), batch_size=30, num_workers=0)
    g = DataLoader(SyntheticPairs(60, seq_len, seed=2), batch_size=30, num_workers=0)
    return train, 625, loader, q, g


def decode_mode():
    """``GRL_DECODE``: 'device' (default) -- loader workers read the JPEG files, the GPU decodes them; 'host' -- Pillow
    decodes in the workers (the escape hatch for streams the device decoder refuses)."""
    mode = os.environ.get('GRL_DECODE', 'device')
    if mode not in ('device', 'host'):
        raise ValueError("GRL_DECODE must be 'device' or 'host', not %r" % mode)
    return mode


def _video_data(name, data_dir, batch_size, seq_len, workers, only_eval):
    """The reference's MARS / Duke branch (dataloader.py:45-81) on RawVideoDataset: the transform chain
    RectScale(256, 128) / flip / erase / ToTensor / Normalize runs on the device."""
    from grl_amd import dist as grl_dist
    from grl_amd.reid.dataset import get_sequence
    from .jpeg import jpeg_collate

    dataset = get_sequence(name, data_dir=data_dir)
    decode = decode_mode()
    host = decode == 'host'
    kw = dict(collate_fn=None if host else jpeg_collate, pin_memory=host and torch.cuda.is_available())

    def frames(tracklets, sample, augment=False):
        # host decode: frames of another size (Duke) are RectScale'd in the worker so that a batch stacks
        return RawVideoDataset(tracklets, seq_len=seq_len, sample=sample, augment=augment, decode=decode,
                               host_rect_scale=host)

    sampler = RandomPairSamplerForMars(dataset.train)
    local_batch, sharded = batch_size, grl_dist.is_distributed()
    if sharded:         # every rank draws the global sequence and keeps its own pairs
        sampler = grl_dist.ShardedPairSampler(sampler, batch_size)
        local_batch = batch_size // torch.distributed.get_world_size()
    train_loader = DataLoader(frames(dataset.train, 'rrs_train', augment=True), batch_size=local_batch,
                              sampler=sampler, num_workers=workers, drop_last=True, **kw)
    train_loader.grl_rank_sharded = sharded
    sample, eval_batch = ('dense', 1) if only_eval else ('rrs_test', 30)
    query_loader = DataLoader(frames(dataset.query, sample), batch_size=eval_batch, shuffle=False,
                              num_workers=workers, drop_last=False, **kw)
    gallery_loader = DataLoader(frames(dataset.gallery, sample), batch_size=eval_batch, shuffle=False,
                                num_workers=workers, drop_last=False, **kw)
    return dataset, dataset.num_train_pids, train_loader, query_loader, gallery_loader


class RawVideoDataset(Dataset):
    """Tracklets -> RAW uint8 clips for the on-device input pipeline (the counterpart of the
    reference's VideoDataset + T.Compose, reid/data/video_loader.py:18-155, dataloader.py:51-72):
    the worker only decodes; RectScale, flip, erase, ToTensor and Normalize run on the GPU.

    ``tracklets``: [(img_paths, pid, camid)] as the reference's dataset objects provide
    (reid/dataset/mars.py); ``sample``: 'rrs_train' | 'rrs_test' | 'dense' with the reference's frame
    selection (``augment.sample_frame_indices``).  Items: (uint8 [T,3,H,W], pid, camid) -- 'dense':
    [n_clips,T,3,H,W] -- plus, with ``augment=True`` (training), the int32 block of
    ``augment.draw_clip_params`` that SEQTrainer hands to grl_augment_normalize_u8.  MARS crops are all
    256 x 128; another uniform size is RectScale'd on the device; frames of DIFFERENT sizes (DukeMTMC-VideoReID):
    see ``host_rect_scale`` below.  With ``index=True`` every item ends with its dataset index (int64, after the
    augmentation block when there is one): the memory row of the sample for ``HybridSEQTrainer``."""

    def __init__(self, tracklets, seq_len=4, sample='rrs_train', augment=False, height=256, width=128, decode='host',
                 host_rect_scale=False, index=False):
        """``decode``: 'host' -- the worker decodes with Pillow (items carry uint8 tensors); 'device' -- the worker only
        reads the files, items carry the JPEG byte strings, the loader uses ``jpeg.jpeg_collate`` and
        engine.DevicePrefetcher decodes the batch on the GPU (grl_jpeg_decode_batch, bit-identical to Pillow).
        ``host_rect_scale``: datasets whose frames DIFFER in size (DukeMTMC-VideoReID) cannot be stacked raw: with
        decode='host' the worker then applies RectScale(height, width) itself (PIL BILINEAR, as the reference); with
        decode='device' nothing is needed -- the prefetcher decodes per size and resizes on the GPU, the same bits."""
        if decode not in ('host', 'device'):
            raise ValueError("decode must be 'host' or 'device'")
        self.tracklets, self.seq_len, self.sample = list(tracklets), seq_len, sample
        self.augment, self.height, self.width, self.decode = augment, height, width, decode
        self.host_rect_scale = host_rect_scale
        self.index = index

    def __len__(self):
        return len(self.tracklets)

    def _decode(self, path):
        import numpy as np
        from PIL import Image
        with Image.open(path) as im:
            im = im.convert('RGB')
            if self.host_rect_scale and im.size != (self.width, self.height):
                im = im.resize((self.width, self.height), Image.BILINEAR)          # seqtransforms.py:30-47
            return torch.from_numpy(np.ascontiguousarray(np.asarray(im).transpose(2, 0, 1)))

    def __getitem__(self, index):
        from .augment import draw_clip_params, sample_frame_indices
        paths, pid, camid = self.tracklets[index]
        idx = sample_frame_indices(len(paths), self.seq_len, self.sample)
        if self.decode == 'device':
            from .jpeg import read_file
            # (each byte string carries its file's path: a frame the device decoder refuses is reported by name)
            if self.sample == 'dense':          # [n_clips][T] byte strings (test_all.py's mode: video_loader.py:86-123)
                item = ([[read_file(paths[int(i)], keep_path=True) for i in row] for row in idx], pid, camid)
            else:
                item = ([read_file(paths[int(i)], keep_path=True) for i in idx], pid, camid)
            if self.augment:
                item += (torch.tensor(draw_clip_params(self.seq_len, self.height, self.width), dtype=torch.int32),)
            if self.index:
                item += (torch.tensor(int(index), dtype=torch.int64),)
            return item
        if self.sample == 'dense':
            clip = torch.stack([torch.stack([self._decode(paths[int(i)]) for i in row]) for row in idx])
        else:
            clip = torch.stack([self._decode(paths[int(i)]) for i in idx])
        item = (clip, pid, camid)
        if self.augment:
            item += (torch.tensor(draw_clip_params(self.seq_len, self.height, self.width), dtype=torch.int32),)
        if self.index:
            item += (torch.tensor(int(index), dtype=torch.int64),)
        return item
