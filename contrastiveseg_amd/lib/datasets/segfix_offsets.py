"""Boundary offsets of the SegFix refinement (test.segfix_offset_dir, this project's own key): one file per image, <dir>/<stem>.mat as
the reference's scripts/cityscapes/segfix.py reads it (scipy.io.loadmat(...)['mat']: [h, w, 2], index 0 the row offset, index 1 the
column offset; the published files hold -1, 0, 1) or <dir>/<stem>.npy with the same array -- this project's addition, so that
nobody needs scipy who does not have .mat files. An integer array whose values fit int8 travels to the device as int8 (a quarter
of the bytes of the reference's float32 copy; kernels.segfix_shift gives identical output for equal values), anything else as float32
(the reference's .astype(np.float32))."""
import os

import numpy as np

# the reference script hard-codes this list (LabelTransformer.label_list); its ADE20K variant is another script
LABEL_LIST = [7, 8, 11, 12, 13, 17, 19, 20, 21, 22, 23, 24, 25, 26, 27, 28, 31, 32, 33]
EXTENSIONS = ('.mat', '.npy')                 # looked for in this order


def find_offset_file(offset_dir, stem):
    """-> <offset_dir>/<stem>.mat, else <offset_dir>/<stem>.npy, else None."""
    for ext in EXTENSIONS:
        path = os.path.join(offset_dir, stem + ext)
        if os.path.exists(path):
            return path
    return None


def _read(path):
    if path.endswith('.mat'):
        try:
            import scipy.io as sio                         # only where a .mat file is actually read
        except ImportError:
            raise ImportError('test.segfix_offset_dir: {} is a MATLAB file and scipy is not installed; install scipy or store the '
                              "array of its 'mat' key as {}.npy".format(path, os.path.splitext(path)[0]))
        mat = sio.loadmat(path)
        if 'mat' not in mat:
            raise ValueError("{}: no variable 'mat' (the offsets [h, w, 2]); the file holds {}"
                             .format(path, sorted(k for k in mat if not k.startswith('__'))))
        return np.asarray(mat['mat'])
    return np.load(path, allow_pickle=False)


def load_offsets(path, shape):
    """-> the offsets of one image as a contiguous int8 or float32 [h, w, 2] array. shape: the image's own (h, w). Refused by name: an
    array of another shape, a non-numeric array, non-finite values."""
    arr = _read(path)
    h, w = int(shape[0]), int(shape[1])
    if arr.shape != (h, w, 2):
        raise ValueError('{}: the offsets are an array of shape {}, the image is {} x {}: expected [{}, {}, 2] (row offset, column '
                         'offset per pixel)'.format(path, tuple(arr.shape), h, w, h, w))
    if arr.dtype.kind not in 'iuf':
        raise ValueError('{}: the offsets are of type {}, expected an integer or floating-point array'.format(path, arr.dtype))
    if arr.dtype.kind == 'f':
        if not np.isfinite(arr).all():
            raise ValueError('{}: the offsets hold {} non-finite values'.format(path, int((~np.isfinite(arr)).sum())))
        return np.ascontiguousarray(arr, dtype=np.float32)
    if arr.size == 0 or (int(arr.min()) >= -128 and int(arr.max()) <= 127):
        return np.ascontiguousarray(arr, dtype=np.int8)
    return np.ascontiguousarray(arr, dtype=np.float32)


def batch_offsets(arrays, regions, size):
    """arrays: one load_offsets result per image, regions: (x0, y0, bw, bh) per image, size: (H, W) of the padded batch -> [B,H,W,2],
    every image's offsets at its region, zero in the padding; int8 when every array is, float32 otherwise."""
    H, W = int(size[0]), int(size[1])
    dtype = np.int8 if all(a.dtype == np.int8 for a in arrays) else np.float32
    out = np.zeros((len(arrays), H, W, 2), dtype=dtype)
    for k, (a, (x0, y0, bw, bh)) in enumerate(zip(arrays, regions)):
        if a.shape != (bh, bw, 2):
            raise ValueError('the offsets of image {} of the batch are {}, its region {} x {}'.format(k, tuple(a.shape), bh, bw))
        out[k, y0:y0 + bh, x0:x0 + bw] = a
    return out
