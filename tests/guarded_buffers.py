"""The buffer contract of a C-API call, checked from outside (tests/test_gpu_buffers.py): every buffer is exactly as large
as the header says, starts at the least alignment its element type allows and lies inside a larger allocation whose
other bytes are known, so that a store past an end, an element never written, a value fetched from beyond an input and a
need for more than natural alignment all show.

    inputs    name -> array.  The array sits in the middle of an allocation whose other bytes are poison: poison "A" is
              0xFF bytes (a NaN where floats are read), poison "B" 0x00 bytes, for floats +3e38.  After the call the whole
              allocation is byte for byte what it was.
    outputs   name -> (dtype, element count).  The elements sit between two runs of GUARD elements; every byte of the
              allocation, the output's own included, starts as SENTINEL.  After the call the output equals the expected
              array bit for bit (floats are compared as their bytes) and every byte outside it is still SENTINEL.
              name -> (dtype, element count, initial array): the output starts as that array instead (a buffer the call
              accumulates into, such as the Monte-Carlo counters); the bytes outside it are SENTINEL all the same.
    addresses bytes at an odd address, 16-bit elements at 2 mod 4, 32-bit elements at 4 mod 8, 64-bit elements at 8 mod 16
              -- asserted before the call.

check_call() makes the call once per subset of the optional outputs (an absent output is a null pointer and has no buffer
at all; outputs named together in a tuple, such as the two arrays of a CSR, are absent only together) with poison A, once
more with every output and poison B, and requires the two full calls to agree bit for bit: a result that depends on what
lies beyond an input's end would differ (a call without inputs has no second poison to meet).  A read past an end whose
value is never used cannot be seen this way.

torch is imported inside the functions: the module loads without a GPU, and device="cpu" runs the same checks on host
memory (the host-pointer entry points)."""
import ctypes as C
import itertools

import numpy as np

GUARD, SENTINEL = 8, 0x5A
PAD = 64  # elements of poison on either side of an input: more than the widest vector access (16 bytes) can cross


def _torch_dtype(torch, dtype):
    """the torch type with the element size and kind of a numpy type (torch has no unsigned 16 / 32 / 64-bit arithmetic)"""
    dtype = np.dtype(dtype)
    table = {np.dtype(np.uint8): torch.uint8, np.dtype(np.uint16): torch.int16, np.dtype(np.int16): torch.int16,
             np.dtype(np.int32): torch.int32, np.dtype(np.uint32): torch.int32, np.dtype(np.float32): torch.float32,
             np.dtype(np.uint64): torch.int64, np.dtype(np.int64): torch.int64}
    return table[dtype]


def _allocate(torch, count, dtype, lead, tail, device):
    """lead + 1 + count + tail elements (lead even); the `count` wanted begin at element lead + 1, which is the least
    aligned address of the type because the allocators hand out blocks aligned to 16 bytes and more"""
    assert lead % 2 == 0
    whole = torch.empty(lead + 1 + count + tail, dtype=_torch_dtype(torch, dtype), device=device)
    view = whole[lead + 1: lead + 1 + count]
    size = whole.element_size()
    assert whole.data_ptr() % 16 == 0
    assert count == 0 or view.data_ptr() % (2 * size) == size, (hex(view.data_ptr()), size)
    return whole, view


def poisoned(torch, array, poison, device="cuda"):
    """`array` in the middle of an allocation filled with `poison`: (whole, view)"""
    array = np.ascontiguousarray(array)
    whole, view = _allocate(torch, array.size, array.dtype, PAD, PAD, device)
    if poison == "A":
        whole.view(torch.uint8).fill_(0xFF)
    elif array.dtype == np.float32:
        whole.fill_(3e38)
    else:
        whole.view(torch.uint8).fill_(0)
    if array.size:
        view.view(torch.uint8).copy_(torch.from_numpy(array.reshape(-1).view(np.uint8).copy()))
    return whole, view


def guarded(torch, count, dtype, device="cuda", initial=None):
    """count elements between two runs of GUARD elements, every byte SENTINEL -- or, inside the view, the bytes of the
    array `initial`: (whole, view)"""
    whole, view = _allocate(torch, count, dtype, GUARD, GUARD, device)
    whole.view(torch.uint8).fill_(SENTINEL)
    if initial is not None:
        flat = np.ascontiguousarray(initial).reshape(-1)
        assert flat.size == count and flat.dtype.itemsize == view.element_size()
        if count:
            view.view(torch.uint8).copy_(torch.from_numpy(flat.view(np.uint8).copy()))
    return whole, view


def guards_intact(torch, whole, view):
    """every byte of `whole` outside `view` is SENTINEL"""
    b = whole.view(torch.uint8)
    first = view.data_ptr() - whole.data_ptr()
    last = first + view.numel() * view.element_size()
    return bool((b[:first] == SENTINEL).all()) and bool((b[last:] == SENTINEL).all())


def _bytes_equal(torch, view, want):
    """view (a tensor) holds the bytes of want (a numpy array)"""
    want = np.ascontiguousarray(want).reshape(-1)
    if view.numel() != want.size or view.element_size() != want.dtype.itemsize:
        return False
    return bool(torch.equal(view.view(torch.uint8).cpu(), torch.from_numpy(want.view(np.uint8))))


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def check_call(call, inputs, outputs, expected, optional=(), absent=(), in_place=None, device="cuda", what=""):
    """Runs `call` under the buffer contract of this module's docstring.

    call(ptrs)  one call of the library: ptrs maps every input and output name to a c_void_p (None for an output that is
                absent) and "stream" to the current torch stream (None on the host); returns the call's status code
    inputs      name -> numpy array
    outputs     name -> (numpy dtype, element count), or (numpy dtype, element count, the array the output starts as)
    expected    name -> the numpy array the output must equal bit for bit, or a function check(tensor, label) that
                asserts what is known of it (a sample of a batch too large for the checker)
    optional    the outputs that may be absent: every subset of them is absent in turn; a tuple of names stands for
                outputs that are absent only together
    absent      outputs that are null in every call (their names still reach `call`, as None)
    in_place    {output: input}: the output is the input's buffer, which then lies between guards
    Returns the outputs of the call with every output present, name -> tensor."""
    import torch
    from channelcoding_amd import capi
    in_place = dict(in_place or {})
    groups = [(g,) if isinstance(g, str) else tuple(g) for g in optional]
    named = [k for g in groups for k in g]
    assert len(set(named)) == len(named) and set(named) <= set(outputs), optional
    groups.sort(key=lambda g: min(list(outputs).index(k) for k in g))  # the order of `outputs`, as before
    assert not set(absent) & set(named) and set(expected) >= set(outputs) - set(absent)

    def one(missing, poison):
        label = (what, "without " + "+".join(missing) if missing else "all outputs", "poison " + poison)
        ins, outs = {}, {}
        for name, array in inputs.items():
            if name in in_place.values():
                whole, view = guarded(torch, array.size, array.dtype, device)
                flat = np.ascontiguousarray(array).reshape(-1)
                view.view(torch.uint8).copy_(torch.from_numpy(flat.view(np.uint8).copy()))
            else:
                whole, view = poisoned(torch, array, poison, device)
            ins[name] = (whole, view)
        for name, (dtype, count, *initial) in outputs.items():
            if name in missing or name in absent:
                outs[name] = None
            elif name in in_place:
                outs[name] = ins[in_place[name]]
                assert np.dtype(dtype) == inputs[in_place[name]].dtype and count == inputs[in_place[name]].size
            else:
                outs[name] = guarded(torch, count, dtype, device, *initial)
        before = {name: whole.view(torch.uint8).clone() for name, (whole, _) in ins.items()
                  if name not in in_place.values()}
        ptrs = {name: _ptr(view) for name, (_, view) in ins.items()}
        ptrs.update({name: None if b is None else _ptr(b[1]) for name, b in outs.items()})
        on_gpu = device != "cpu"
        ptrs["stream"] = C.c_void_p(torch.cuda.current_stream().cuda_stream) if on_gpu else None
        for name, b in list(ins.items()) + [(k, v) for k, v in outs.items() if v is not None]:
            size = b[1].element_size()
            assert b[1].numel() == 0 or b[1].data_ptr() % (2 * size) == size, (label, name)  # the least alignment
        capi.check(call(ptrs), str(label))
        if on_gpu:
            torch.cuda.synchronize()
        for name, b in outs.items():
            if b is None:
                continue
            whole, view = b
            assert guards_intact(torch, whole, view), (label, name, "a byte outside the buffer was written")
            want = expected[name]
            if callable(want):
                want(view, (label, name))
            else:
                assert _bytes_equal(torch, view, want), (label, name, "differs from the expected array")
        for name, image in before.items():
            assert torch.equal(ins[name][0].view(torch.uint8), image), (label, name, "an input was written")
        return {name: b[1] for name, b in outs.items() if b is not None}

    full = one((), "A")
    for r in range(1, len(groups) + 1):
        for chosen in itertools.combinations(groups, r):
            one(tuple(k for g in chosen for k in g), "A")
    if not inputs:  # nothing to read beyond: the second poison would repeat the first call
        return full
    other = one((), "B")
    for name in full:
        assert torch.equal(full[name].view(torch.uint8), other[name].view(torch.uint8)), \
            (what, name, "the result depends on memory outside the inputs")
    return full
