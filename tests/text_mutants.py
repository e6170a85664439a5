"""Wrong restatements of the text model, made by substituting text in a function's source (test infrastructure).

A table maps a name to (function of tests/cuda_text_model.py, text, replacement, which occurrence - None: the only one, "all":
every one).  `mutant(table, name)` compiles the changed source in a copy of the model's namespace and puts the result in the
function's place for the duration of the block: callers inside the model (the shader calls the shadow sum) see it as well.
Shared by tests/test_primitive_edge_cases.py and tests/test_shader_edge_cases.py."""
import contextlib
import inspect

import cuda_text_model as M


@contextlib.contextmanager
def mutant(table, name, extra=None):
    func, old, new, nth = table[name]
    original = getattr(M, func)
    src = inspect.getsource(original)
    count = src.count(old)
    if nth is None:
        assert count == 1, (name, count)
        src = src.replace(old, new)
    elif nth == "all":
        assert count >= 1, name
        src = src.replace(old, new)
    else:
        assert count > nth, (name, count)
        parts = src.split(old)
        src = old.join(parts[: nth + 1]) + new + old.join(parts[nth + 1:])
    space = dict(vars(M), **(extra or {}))
    exec(compile(src, "<mutant %s>" % name, "exec"), space)
    made = space[func]
    setattr(M, func, made)
    try:
        yield
    finally:
        setattr(M, func, original)
