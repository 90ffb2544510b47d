"""ctypes binding of libvibo_hip.so.  The C ABI is declared in include/vibo_hip.h and read from there: every export's
restype / argtypes come from its prototype (parse_prototypes); the constants and the two structs mirror the header by hand
(tests/test_capi_symbols.py compares them).  Exports declared in a header of their own beside it (EXTRA_HEADERS:
vibo_hip_decoder_multi.h, vibo_hip_sign_rows.h, vibo_hip_person_tables.h, vibo_hip_tile_rows.h, vibo_hip_given_tiles.h,
vibo_hip_sparse_rows.h, vibo_hip_sparse_gather.h, vibo_hip_sparse_row_driven.h) are bound the same way; EXPORTED_SYMBOLS stays the list of vibo_hip.h itself,
EXTRA_SYMBOLS, SIGN_ROWS_SYMBOLS, PERSON_TABLE_SYMBOLS, TILE_ROWS_SYMBOLS, GIVEN_TILES_SYMBOLS, SPARSE_ROWS_SYMBOLS,
SPARSE_GATHER_SYMBOLS and SPARSE_ROW_DRIVEN_SYMBOLS are theirs.

The product path has no CPU or eager-PyTorch fallback: if the HIP library is
missing or a call fails, this module raises.
"""
import ctypes
import os
import re

ABI_VERSION = 2
NUM_SCALARS = 8
S_LL, S_REG, S_KL, S_LOGQ0, S_LOGP, S_LADJ, S_NOBS = 0, 1, 2, 3, 4, 5, 6

IRT_1PL, IRT_2PL, IRT_3PL = 1, 2, 3
POSTERIOR_UNCONDITIONAL, POSTERIOR_CONDITIONAL, POSTERIOR_GIVEN = 0, 1, 2
MISSING_PRIOR, MISSING_DROP = 0, 1
MASK_U8, MASK_I64, MASK_NONE, MASK_CODES = 0, 1, 2, 3
MASK_SIGN = 4                 # include/vibo_hip_sign_rows.h: no mask, the response's sign bit says "missing"
MASK_TILES = 6                # include/vibo_hip_tile_rows.h: `response` is the matrix' prepacked tile image, no mask
TILE_WAVE_BLOCK_BYTES = 4352  # ... one wave's 128 items x 32 rows: 16 code words and a counts dword per lane
# include/vibo_hip_sparse_rows.h: the matrix as its observed cells (VIBO_SPARSE_*)
SPARSE_CHUNK, SPARSE_ROWS_PER_BLOCK, SPARSE_MAX_BLOCKS, SPARSE_RECORD_FLOATS = 512, 32, 1024, 72
SPARSE_NO_SLOT = 0x7fffffff   # include/vibo_hip_sparse_gather.h: a person_slot entry no row of a gathered call owns
REG_KL, REG_SAMPLED = 0, 1
FLAG_KERNEL_VALU, FLAG_KERNEL_MATRIX, FLAG_NO_EMIT_CODES, FLAG_COND_VALU, FLAG_COND_MATRIX, FLAG_COND_THREE_PASS = 1, 2, 4, 8, 16, 32
KERNEL_NAMES = {1: 'matrix row-split (msplit_kernel)', 2: 'VALU row-split (split_kernel)', 3: 'wave-per-row', 4: 'tiled',
                5: 'wave-per-person', 6: 'narrow rows (narrow_kernel)'}
MAX_ABILITY_DIM = 16          # vibo_elbo_fwd_bwd / vibo_encode / vibo_decode (9..16: the wave-per-person kernel)
MAX_ABILITY_DIM_FAST = 8      # row-split / matrix-pipe kernels, trainers' native conditional / flow step, mean merge
MAX_FLOWS = 8
DECODER_KINDS = {'link': 1, 'deep': 2, 'residual': 3}      # VIBO_DECODER_*
DTRAIN_SCALARS, DTRAIN_POSTERIOR, DTRAIN_ABILITY = 0, 1, 2

LIB_NAME = 'libvibo_hip.so'
# VIBO_HIP_LIB points at another build of the same ABI (A/B timing of kernel variants); default: the in-tree build
LIB_PATH = os.environ.get('VIBO_HIP_LIB') or os.path.join(os.path.dirname(os.path.abspath(__file__)), LIB_NAME)


class ViboDesc(ctypes.Structure):
    """struct vibo_desc (include/vibo_hip.h)."""
    _fields_ = [
        ('abi_version', ctypes.c_int32),
        ('num_person', ctypes.c_int32),
        ('num_item', ctypes.c_int32),
        ('ability_dim', ctypes.c_int32),
        ('irt_model', ctypes.c_int32),
        ('posterior', ctypes.c_int32),
        ('missing_mode', ctypes.c_int32),
        ('mask_dtype', ctypes.c_int32),
        ('reg_mode', ctypes.c_int32),
        ('n_flows', ctypes.c_int32),
        ('want_grad', ctypes.c_int32),
        ('deterministic', ctypes.c_int32),
        ('response_row_stride', ctypes.c_int64),
        ('mask_row_stride', ctypes.c_int64),
        ('flags', ctypes.c_int32),
        ('reserved', ctypes.c_int32),
    ]


class ViboDecoderDesc(ctypes.Structure):
    """struct vibo_decoder_desc (include/vibo_hip.h)."""
    _fields_ = [
        ('num_person', ctypes.c_int32),
        ('num_item', ctypes.c_int32),
        ('hidden_dim', ctypes.c_int32),
        ('want_grad', ctypes.c_int32),
        ('person_chunks', ctypes.c_int32),
        ('resid', ctypes.c_float),
        ('response_row_stride', ctypes.c_int64),
        ('mask_row_stride', ctypes.c_int64),
    ]


class ViboSparseImage(ctypes.Structure):
    """struct vibo_sparse_image (include/vibo_hip_sparse_rows.h); the pointers are device pointers."""
    _fields_ = [
        ('num_person', ctypes.c_int64),
        ('num_item', ctypes.c_int64),
        ('nnz', ctypes.c_int64),
        ('num_chunk', ctypes.c_int64),
        ('row_ptr', ctypes.c_void_p),
        ('row_cell', ctypes.c_void_p),
        ('col_ptr', ctypes.c_void_p),
        ('col_cell', ctypes.c_void_p),
        ('col_chunk', ctypes.c_void_p),
        ('chunk_item', ctypes.c_void_p),
        ('chunk_first', ctypes.c_void_p),
    ]


HEADER_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', '..', 'include', 'vibo_hip.h')
_SCALAR_TYPES = {'int': ctypes.c_int, 'int32_t': ctypes.c_int32, 'uint32_t': ctypes.c_uint32, 'int64_t': ctypes.c_int64,
                 'uint64_t': ctypes.c_uint64, 'size_t': ctypes.c_size_t}
_DESC_TYPES = {'vibo_desc': ViboDesc, 'vibo_decoder_desc': ViboDecoderDesc, 'vibo_sparse_image': ViboSparseImage}


class ViboLibraryError(RuntimeError):
    pass


def parse_prototypes(header):
    """[(name, restype, argtypes)] of every `ret vibo_name(params);` of the header's text, in its order: the one statement of the
    C ABI this binding has.  Descriptor pointers are typed, every other pointer is a void*, scalars go by their C type; a type
    that is not in the tables above is an error, never a default."""
    def ctype(c_type, name, is_return=False):
        base = ' '.join(w for w in c_type.replace('*', ' * ').split() if w != 'const')
        if base == 'char *' and is_return:
            return ctypes.c_char_p
        if base.endswith(' *') and not is_return:
            return ctypes.POINTER(_DESC_TYPES[base[:-2]]) if base[:-2] in _DESC_TYPES else ctypes.c_void_p
        if base not in _SCALAR_TYPES:
            raise ViboLibraryError(f'include/vibo_hip.h: {name}: no ctypes mapping for the type "{c_type.strip()}"')
        return _SCALAR_TYPES[base]

    protos = []
    text = re.sub(r'/\*.*?\*/', '', header, flags=re.S)
    for ret, name, params in re.findall(r'^[ \t]*([\w \t]+?[ \t*]+)(vibo_\w+)\s*\(([^()]*)\)\s*;', text, flags=re.M):
        params = [] if params.strip() in ('', 'void') else params.split(',')
        # (a parameter is `type name`: the name is the last word)
        protos.append((name, ctype(ret, name, True), [ctype(re.sub(r'\w+\s*$', '', p), name) for p in params]))
    return protos


EXTRA_HEADERS = ('vibo_hip_decoder_multi.h', 'vibo_hip_sign_rows.h', 'vibo_hip_person_tables.h', 'vibo_hip_tile_rows.h',
                 'vibo_hip_given_tiles.h', 'vibo_hip_sparse_rows.h', 'vibo_hip_sparse_gather.h', 'vibo_hip_sparse_row_driven.h')

with open(HEADER_PATH) as _header:
    PROTOTYPES = parse_prototypes(_header.read())
EXPORTED_SYMBOLS = tuple(name for name, _, _ in PROTOTYPES)
EXTRA_PROTOTYPES = []
_HEADER_SYMBOLS = {}
for _name in EXTRA_HEADERS:
    with open(os.path.join(os.path.dirname(HEADER_PATH), _name)) as _header:
        _protos = parse_prototypes(_header.read())
    EXTRA_PROTOTYPES += _protos
    _HEADER_SYMBOLS[_name] = tuple(name for name, _, _ in _protos)
# (one list per header: EXTRA_SYMBOLS is vibo_hip_decoder_multi.h's, as its tests pin it)
EXTRA_SYMBOLS = _HEADER_SYMBOLS['vibo_hip_decoder_multi.h']
SIGN_ROWS_SYMBOLS = _HEADER_SYMBOLS['vibo_hip_sign_rows.h']
PERSON_TABLE_SYMBOLS = _HEADER_SYMBOLS['vibo_hip_person_tables.h']      # the VI / MLE train step (trainer.FusedVITrainer / FusedMLETrainer)
TILE_ROWS_SYMBOLS = _HEADER_SYMBOLS['vibo_hip_tile_rows.h']
GIVEN_TILES_SYMBOLS = _HEADER_SYMBOLS['vibo_hip_given_tiles.h']          # the tile image under a caller-supplied posterior (ops._tile_rows)
SPARSE_ROWS_SYMBOLS = _HEADER_SYMBOLS['vibo_hip_sparse_rows.h']          # the matrix as its observed cells (vibo_amd/sparse.py)
SPARSE_GATHER_SYMBOLS = _HEADER_SYMBOLS['vibo_hip_sparse_gather.h']      # ... for an index vector of persons (SparseRows.take)
SPARSE_ROW_DRIVEN_SYMBOLS = _HEADER_SYMBOLS['vibo_hip_sparse_row_driven.h']  # ... with the row-driven item pass (item_pass='rows')
PTRAIN_VI, PTRAIN_MLE = 0, 1                                            # VIBO_PTRAIN_*
PTRAIN_MAX_BLOCKS = 2048                                                # VIBO_PTRAIN_MAX_BLOCKS: the table update's grid cap

_lib = None


def load():
    """Load (once) and return the ctypes handle, every export typed from the header; raises if the library is absent."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ViboLibraryError(
            f'{LIB_PATH} not found: build the HIP extension first '
            f'(python __graft_entry__.py, or make -C variational-item-response-theory-public_amd/csrc). '
            f'There is no CPU fallback.')
    lib = ctypes.CDLL(LIB_PATH)
    for name, restype, argtypes in PROTOTYPES + EXTRA_PROTOTYPES:
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = restype, argtypes
    if lib.vibo_version() != ABI_VERSION:
        raise ViboLibraryError(f'ABI mismatch: library {lib.vibo_version()} != binding {ABI_VERSION}')
    _lib = lib
    return lib


def check(rc, what):
    if rc != 0:
        msg = load().vibo_last_error_string().decode('utf-8', 'replace')
        raise ViboLibraryError(f'{what} failed (rc={rc}): {msg}')
