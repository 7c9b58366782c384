"""TEST INFRASTRUCTURE — CPU restatement of one training batch of ptt_amd.train_feed.TrainBatchFeeder from (tracklets,
settings, seed, epoch, batch): the reference's get_train_items (ptt/datasets/kitti/kitti_dataset_tracking.py:60-179) per
candidate on oracle.tracking_ref, numpy's own multivariate_normal / uniform on RandomState([seed, epoch, index]), a Philox4x32-10
written out in numpy, and the replacement rule of include/ptt_hip.h (N5). Nothing here imports the product."""
import copy

import numpy as np

from oracle import tracking_ref as TR

DEFAULTS = dict(batch_size=48, search_size=1024, template_size=512, search_offset=0.0, search_scale=1.25, model_offset=0.0,
                model_scale=1.25, use_z=True, refine_box=True, candidates_per_frame=4, sampled_interval=1, min_points=20, spare=None,
                shuffle=True, drop_last=True, rank=0, world=1)


def settings(**kw):
    s = dict(DEFAULTS, **kw)
    if s['spare'] is None:
        s['spare'] = max(4, s['batch_size'] // 8)
    return s


# ------------------------------------------------------------------ Philox4x32-10
def philox4x32_10(counter, key):
    """counter (..., 4), key (..., 2) uint32 -> (..., 4) uint32 (Salmon et al., SC'11: ten rounds, Weyl key schedule)."""
    c = [np.asarray(counter, np.uint64)[..., k] for k in range(4)]
    k0, k1 = (np.broadcast_to(np.asarray(key, np.uint64)[..., k], c[0].shape).copy() for k in range(2))
    m32 = np.uint64(0xffffffff)
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c[0], np.uint64(0xCD9E8D57) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k0, p1 & m32, (p0 >> np.uint64(32)) ^ c[3] ^ k1, p0 & m32]
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & m32, (k1 + np.uint64(0xBB67AE85)) & m32
    return np.stack(c, -1).astype(np.uint32)


def draw_indices(n, size, index, which, epoch, seed):
    """The `size` resampling indices in [0, n) of (dataset index, which = 0 search / 1 template, epoch) under `seed`: draw i = word
    i & 3 of block i >> 2, scaled by (word * n) >> 32."""
    blocks = (size + 3) // 4
    ctr = np.zeros((blocks, 4), np.uint64)
    ctr[:, 0], ctr[:, 1], ctr[:, 2], ctr[:, 3] = np.arange(blocks), index, which, epoch
    words = philox4x32_10(ctr, np.array([seed & 0xffffffff, seed >> 32], np.uint64)).reshape(-1)[:size]
    return ((words.astype(np.uint64) * np.uint64(n)) >> np.uint64(32)).astype(np.int64)


# ------------------------------------------------------------------ the index plan
def frame_map(tracklets):
    """get_frame_seq_map (:211-219): annotation index -> (tracklet, frame)."""
    return [(t, i) for t, (clouds, _) in enumerate(tracklets) for i in range(len(clouds))]


def length(tracklets, s):
    return len(frame_map(tracklets)) * s['candidates_per_frame'] // s['sampled_interval']             # __len__ :44-47


def locate(tracklets, s, index):
    """Dataset index -> (tracklet, frame, augmentation) (__getitem__ :51, get_anno_index / get_aug_index :221-225)."""
    full = index * s['sampled_interval']
    t, i = frame_map(tracklets)[int(full / s['candidates_per_frame'])]
    return t, i, int(full % s['candidates_per_frame'])


def shard(n, rank, world):
    """tracklet_shard.shard_indices: arange(n) padded by wrapping to a multiple of world, then rank::world."""
    per = -(-n // world)
    idx = list(range(n))
    while len(idx) < per * world:
        idx += idx[:per * world - len(idx)]
    return idx[rank:per * world:world]


def order(tracklets, s, seed, epoch):
    n = length(tracklets, s)
    perm = np.random.RandomState([seed, epoch]).permutation(n) if s['shuffle'] else np.arange(n)
    return perm[np.array(shard(n, s['rank'], s['world']), np.int64)]


def batch_indices(tracklets, s, seed, epoch, batch):
    """B primaries, then the spares."""
    o, B = order(tracklets, s, seed, epoch), s['batch_size']
    prim = o[(batch * B + np.arange(B)) % len(o)]
    spares = np.random.RandomState([seed, epoch, batch * s['world'] + s['rank']]).randint(0, length(tracklets, s), s['spare'])
    return np.concatenate([prim, spares]).astype(np.int64)


# ------------------------------------------------------------------ one candidate
def _box(b):
    return TR.RefBox(b[0], b[1], b[2])


def _moved(box, offset, use_z, rs):
    """get_box_by_offset (:192-216) -> (the moved box, the offsets as used: the reference overwrites offset[0] / offset[1] in
    place with its redraws)."""
    draws = []

    def uniform():
        draws.append(rs.uniform(-1, 1))
        return draws[-1]

    new_box = TR.get_box_by_offset(box, offset, use_z, uniform=uniform)
    used, k = np.array(offset, np.float64), 0
    if offset[0] > box.wlh[0]:
        used[0], k = draws[k], k + 1
    if offset[1] > min(box.wlh[1], 2):
        used[1] = draws[k]
    return new_box, used


def candidate(tracklets, s, seed, epoch, index):
    """get_train_items of one dataset index, up to (not including) regularize_pc: dict of search_offset, template_offset (3,), search
    (n,3) float32, label (n,) float64, reg (4,) float64, template (m,3) float32, valid."""
    t, i, aug = locate(tracklets, s, int(index))
    clouds, boxes = tracklets[t]
    rs = np.random.RandomState([seed, epoch, int(index)])
    gt = _box(boxes[i])
    off_s = np.zeros(3) if aug == 0 else rs.multivariate_normal(np.zeros(3), np.diag([1, 1, 5]), size=1)[0]       # :121-125
    sample_box, off_s = _moved(gt, off_s, s['use_z'], rs)                                                          # :128
    pts, label = TR.crop_center_pc_labels(clouds[i], sample_box, gt, s['search_offset'], s['search_scale'], s['refine_box'])
    # label_reg (:310-325): the ground-truth box carried through the sample box's translate / rotate
    g = copy.deepcopy(gt)
    g.translate(-sample_box.center)
    g.rotate(TR._Quat.from_matrix(np.transpose(sample_box.rotation_matrix)))
    reg = np.array([g.center[0], g.center[1], g.center[2], -off_s[-1]])
    if aug == 0:                                                                                                   # :152-156
        off_t = np.zeros(3)
    else:
        off_t = rs.uniform(low=-0.3, high=0.3, size=3)
        off_t[2] = off_t[2] * 5.0
    p = max(i - 1, 0)
    prev_box, off_t = _moved(_box(boxes[p]), off_t, s['use_z'], rs)                                                # :160
    model = TR.get_model([clouds[0], clouds[p]], [_box(boxes[0]), prev_box], s['model_offset'], s['model_scale'])   # :168-174
    search, template = np.ascontiguousarray(pts.T, np.float32), np.ascontiguousarray(model.T, np.float32)
    valid = search.shape[0] > s['min_points'] and template.shape[0] > s['min_points']                              # :140, :176
    return {'search_offset': off_s, 'template_offset': off_t, 'search': search, 'label': label.astype(np.float64), 'reg': reg,
            'template': template, 'valid': bool(valid)}


# ------------------------------------------------------------------ one batch
def sources(valid, B):
    """The replacement rule: valid (C,) bool -> (src (B,), info = [invalid primaries, valid spares, shortfall, all_invalid])."""
    valid = np.asarray(valid, bool)
    ranked = list(np.nonzero(valid)[0])
    spares = [c for c in ranked if c >= B]
    n_inv = int(B - valid[:B].sum())
    src, r = np.full(B, -1, np.int64), 0
    for b in range(B):
        if valid[b]:
            src[b] = b
            continue
        if ranked:
            src[b] = spares[r] if r < len(spares) else ranked[(r - len(spares)) % len(ranked)]
        r += 1
    return src, np.array([n_inv, len(spares), max(0, n_inv - len(spares)), int(not ranked)], np.int64)


def resample(rows, size, index, which, epoch, seed, label=None):
    """regularize_pc(istrain=True) (kitti_tracking_utils.py:342-367) on the counter-based indices: -> (points (size,3), idx (size,)
    or -1 for a pass-through[, labels])."""
    n = rows.shape[0]
    idx = None if n == size else draw_indices(n, size, index, which, epoch, seed)
    pts = rows if idx is None else rows[idx]
    out = [pts, np.full(size, -1, np.int64) if idx is None else idx]
    if label is not None:
        out.append((label if idx is None else label[idx]).astype(np.float32))
    return out


def batch(tracklets, s, seed, epoch, number, cache=None):
    """cache: a dict the per-candidate results are kept in, keyed by dataset index (one per (tracklets, crop settings, seed, epoch):
    a candidate does not depend on the batch it appears in). -> dict: search_points (B,S,3), template_points (B,T,3), cls_label (B,S), reg_label (B,4) float32; src (B,), idx_search (B,S),
    idx_template (B,T); info (4,); index (C,); candidates (the per-candidate dicts)."""
    B, S, T = s['batch_size'], s['search_size'], s['template_size']
    index = batch_indices(tracklets, s, seed, epoch, number)
    cache = {} if cache is None else cache
    for j in index:
        if int(j) not in cache:
            cache[int(j)] = candidate(tracklets, s, seed, epoch, j)
    cands = [cache[int(j)] for j in index]
    src, info = sources([c['valid'] for c in cands], B)
    out = {'search_points': np.zeros((B, S, 3), np.float32), 'template_points': np.zeros((B, T, 3), np.float32),
           'cls_label': np.zeros((B, S), np.float32), 'reg_label': np.zeros((B, 4), np.float32), 'src': src, 'info': info,
           'idx_search': np.full((B, S), -1, np.int64), 'idx_template': np.full((B, T), -1, np.int64), 'index': index, 'candidates': cands}
    for b in range(B):
        if src[b] < 0:
            continue
        c, j = cands[src[b]], int(index[src[b]])
        out['search_points'][b], out['idx_search'][b], out['cls_label'][b] = resample(c['search'], S, j, 0, epoch, seed, c['label'])
        out['template_points'][b], out['idx_template'][b] = resample(c['template'], T, j, 1, epoch, seed)
        out['reg_label'][b] = c['reg'].astype(np.float32)
    return out
