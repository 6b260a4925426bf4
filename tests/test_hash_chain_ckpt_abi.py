"""The checkpoint calls' C ABI (efes_hash_chain_checkpoints, efes_checkpoints_marshal_text) without a GPU:
the symbols, the record's layout and text size, the argument errors that need no device, and the
DeviceObjects refusal that follows from the arguments alone."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "efes_hash.h")
API = os.path.join(ROOT, "efes_amd", "csrc", "efes_api.cpp")


def test_symbols_exist(efes_lib):
    L = efes_lib.lib()
    assert L.efes_hash_chain_checkpoints and L.efes_checkpoints_marshal_text
    assert "efes_hash_chain_checkpoints" in efes_lib.SIGNATURES and "efes_checkpoints_marshal_text" in efes_lib.SIGNATURES
    header = open(HEADER).read()
    assert re.search(r"\bint\s+efes_hash_chain_checkpoints\s*\(", header)
    assert re.search(r"\bint\s+efes_checkpoints_marshal_text\s*\(", header)


def test_abi_version_stays_8(efes_lib):
    assert efes_lib.lib().efes_abi_version() == 8
    assert re.search(r"#define\s+EFES_ABI_VERSION\s+8\b", open(HEADER).read())


def test_record_layout(efes_lib):
    dt = efes_lib.CHECKPOINT_DTYPE
    assert dt.itemsize == 112
    assert dt.fields["sha1"][0] == efes_lib.SHA1_STATE_DTYPE and dt.fields["sha1"][1] == 0
    assert dt.fields["crc"][1] == 104 and dt.fields["_pad"][1] == 108
    assert re.search(r"static_assert\(sizeof\(efes_checkpoint\) == 112", open(API).read())
    header = open(HEADER).read()
    m = re.search(r"typedef struct efes_checkpoint \{(.*?)\} efes_checkpoint;", header, re.S)
    assert m, "efes_checkpoint is declared in the header"
    fields = re.findall(r"^\s*(\w+)\s+(\w+);", m.group(1), re.M)
    assert fields == [("efes_sha1_state", "sha1"), ("efes_crc32_state", "crc32"), ("uint32_t", "_pad")]


def test_text_bytes(efes_lib):
    assert efes_lib.CHECKPOINT_TEXT_BYTES == 208
    assert re.search(r"#define\s+EFES_CHECKPOINT_TEXT_BYTES\s+208\b", open(HEADER).read())


def _modes(efes_lib):
    return [efes_lib.MODE_DEEP] + [efes_lib.MODE_GROUP[g] for g in (4, 8, 16, 32)]


def test_null_context_is_an_argument_error(efes_lib):
    L = efes_lib.lib()
    job, ptr = efes_lib.Job(), ctypes.c_uint64(0)
    for mode in _modes(efes_lib):
        assert L.efes_hash_chain_checkpoints(None, None, 0, None, None, 0, None, mode) == efes_lib.EFES_ERR_ARG, mode
        assert L.efes_hash_chain_checkpoints(None, ctypes.addressof(job), 1, ctypes.addressof(ptr), None, 0, None,
                                             mode) == efes_lib.EFES_ERR_ARG, mode
    rec, text = (ctypes.c_uint8 * 112)(), (ctypes.c_char * 208)()
    assert L.efes_checkpoints_marshal_text(None, None, 0, None, None) == efes_lib.EFES_ERR_ARG
    assert L.efes_checkpoints_marshal_text(None, ctypes.addressof(rec), 1, ctypes.addressof(text), None) == efes_lib.EFES_ERR_ARG


def _unopened_ctx():
    """A stand-in for a context in the checks below, which must return before the context is used: the
    errors follow from the other arguments alone, so no device is opened.  Returns the buffer (keep it
    alive) and its address."""
    buf = ctypes.create_string_buffer(4096)
    return buf, ctypes.addressof(buf)


def test_null_checkpoint_array_is_an_argument_error(efes_lib):
    """NULL ckpt_device with njobs = 1: refused before the scratch is looked at or anything is launched
    (the scratch here is valid in size and alignment as far as the host can tell)."""
    L = efes_lib.lib()
    job = efes_lib.Job()
    need = L.efes_hash_chain_scratch(1)
    assert need > 0
    scratch = ctypes.create_string_buffer(need + 16)
    s = (ctypes.addressof(scratch) + 15) & ~15
    keep, ctx = _unopened_ctx()
    for mode in _modes(efes_lib):
        assert L.efes_hash_chain_checkpoints(ctx, ctypes.addressof(job), 1, None, s, need, None,
                                             mode) == efes_lib.EFES_ERR_ARG, mode


def test_auto_and_unknown_modes_are_argument_errors(efes_lib):
    L = efes_lib.lib()
    job, ptr = efes_lib.Job(), ctypes.c_uint64(0)
    keep, fake = _unopened_ctx()
    others = [efes_lib.MODE_AUTO, efes_lib.MODE_WIDE, efes_lib.MODE_FED4, efes_lib.MODE_FED4E, -1, 9, 1 << 20]
    for mode in others:
        for ctx in (None, fake):
            for n in (0, 1):
                assert L.efes_hash_chain_checkpoints(ctx, ctypes.addressof(job), n, ctypes.addressof(ptr), None, 0, None,
                                                     mode) == efes_lib.EFES_ERR_ARG, (mode, n)


def test_marshal_text_null_pointers_and_bound(efes_lib):
    L = efes_lib.lib()
    keep, ctx = _unopened_ctx()
    rec, text = (ctypes.c_uint8 * 112)(), (ctypes.c_char * 208)()
    assert L.efes_checkpoints_marshal_text(ctx, None, 1, ctypes.addressof(text), None) == efes_lib.EFES_ERR_ARG
    assert L.efes_checkpoints_marshal_text(ctx, ctypes.addressof(rec), 1, None, None) == efes_lib.EFES_ERR_ARG
    assert L.efes_checkpoints_marshal_text(ctx, ctypes.addressof(rec), efes_lib.EFES_HASH_CHAIN_MAX_JOBS + 1,
                                           ctypes.addressof(text), None) == efes_lib.EFES_ERR_ARG


def test_device_objects_checkpoints_need_sha1():
    from efes_amd import batch
    with pytest.raises(ValueError, match="checkpoints"):
        batch.DeviceObjects(0, [[(0, 16)]], checkpoints=True)
    with pytest.raises(ValueError, match="checkpoints"):
        batch.DeviceObjects(0, [[(0, 16)]], checkpoints=True, crc32=True, sha1=False, running=True)
