"""A numpy model of the tile image of a response matrix (VIBO_MASK_TILES), written from the layout text of
include/vibo_hip_tile_rows.h -- not from the kernel or the builder: cell (row, item) -> its byte of the image, and the counts dwords."""
import numpy as np

WAVE_BLOCK = 4352           # bytes: 4096 of code words | 256 of counts
MISSING, WRONG, RIGHT = 0x00, 0x38, 0xB8


def observed_and_right(response=None, mask=None, codes=None, sign=False):
    """-> (observed, right) bool [P, I] of the source rows as the header defines them per format: fp32 + u8 mask (bytes 0 / 1),
    fp32 without a mask, fp32 whose sign bit is the mask (sign=True), or 1-byte cell codes (0 wrong / 1 right / 2 missing)."""
    if codes is not None:
        c = np.asarray(codes)
        return c != 2, c == 1
    bits = np.ascontiguousarray(np.asarray(response, dtype=np.float32)).view(np.uint32)
    top_bit0 = ((bits >> 24) & 1) == 1                                   # bit 0 of the float's top byte
    if sign:
        obs = (bits >> 31) == 0
    elif mask is None:
        obs = np.ones(bits.shape, dtype=bool)
    else:
        obs = np.asarray(mask) == 1
    return obs, obs & top_bit0


def image_bytes(P, I):
    return WAVE_BLOCK * ((I + 127) // 128) * ((P + 31) // 32)


def build_image(observed, right):
    """The image (uint8 [image_bytes]) of a P x I matrix given which cells are observed and which of those answered right."""
    observed, right = np.asarray(observed, dtype=bool), np.asarray(right, dtype=bool)
    P, I = observed.shape
    W, NB = (I + 127) // 128, (P + 31) // 32
    # the matrix padded to whole batches and whole waves: padding cells are missing and counted nowhere
    obs = np.zeros((NB * 32, W * 128), dtype=bool)
    rgt = np.zeros_like(obs)
    obs[:P, :I], rgt[:P, :I] = observed, right & observed
    byte = np.where(obs, np.where(rgt, RIGHT, WRONG), MISSING).astype(np.uint8)
    image = np.zeros((NB, W, WAVE_BLOCK), dtype=np.uint8)
    words = image[:, :, :4096].reshape(NB, W, 4, 64, 4, 4)                # [bt][q][run k = 2 h + u][lane l][j][byte = item & 3]
    counts = image[:, :, 4096:].reshape(NB, W, 64, 4)                     # [bt][q][lane l][byte of the dword]
    b6 = byte.reshape(NB, 2, 4, 4, W, 2, 16, 4)                           # row = 32 bt + 16 h + 4 g + j; item = 4 (32 q + 16 u + i16) + t
    o6 = obs.reshape(NB, 2, 4, 4, W, 2, 16, 4)                            #  axes: bt, h, g, j, q, u, i16, t
    for h in range(2):
        for u in range(2):
            # run 2 h + u: lane 16 g + i16, word j
            run = b6[:, h, :, :, :, u, :, :]                              # [bt][g][j][q][i16][t]
            words[:, :, 2 * h + u] = run.transpose(0, 3, 1, 4, 2, 5).reshape(NB, W, 64, 4, 4)
    row_obs = obs.reshape(NB, 32, W, 128).sum(axis=3).transpose(0, 2, 1)             # [bt][q][row of the batch]
    row_right = rgt.reshape(NB, 32, W, 128).sum(axis=3).transpose(0, 2, 1)
    own = o6.sum(axis=(1, 3, 5, 7)).transpose(0, 2, 1, 3).reshape(NB, W, 64)         # [bt][g][q][i16] -> lane 16 g + i16: its 64 cells
    lanes = np.arange(64)
    dword = (row_obs[:, :, lanes & 31].astype(np.uint32) | (row_right[:, :, lanes & 31].astype(np.uint32) << 16) |
             (own.astype(np.uint32) << 24))
    counts[...] = dword.astype('<u4').view(np.uint8).reshape(NB, W, 64, 4)
    return image.reshape(-1)


def cell_byte(image, P, I, row, item):
    """The image's byte of cell (row, item), located by the header's offset formula alone (an independent walk of the layout)."""
    W = (I + 127) // 128
    bt, r = divmod(row, 32)
    h, r = divmod(r, 16)
    g, j = divmod(r, 4)
    c, t = divmod(item, 4)
    q, c = divmod(c, 32)
    u, i16 = divmod(c, 16)
    lane = 16 * g + i16
    return int(image[(bt * W + q) * WAVE_BLOCK + 1024 * (2 * h + u) + 16 * lane + 4 * j + t])
