"""The two builds tests/test_fwd_stream_gpu.py compares: the state model's configuration compiled as the tree
has it (the forward streams its weight fragments a phase ahead of their MFMAs, Model::PF_F) and with
-DUDE_FWD_STREAM=0 (every phase issues its own fragments at its head).  Each is a library of its own under the
package's _build/, named by the source hash, so a library of the current sources is reused and the process-wide
state of the prebuilt library (Ops::fwd_res reads UDE_FWD_RES once) plays no part."""
import os
from concurrent.futures import ThreadPoolExecutor

from conftest import import_pkg

import_pkg()                                         # puts ude_amd on sys.path
from ude_amd import _native, configs  # noqa: E402

CFG = configs._c("FaFp", 49, 8, [64, 64, 32], [64, 64])
FLAGS = {"on": [], "off": ["-DUDE_FWD_STREAM=0"]}


def lib_path(which):
    return os.path.join(_native.BUILD, f"libude_rk4_fwdstream_{which}_{_native.source_hash()[:10]}.so")


def build_libraries():
    """{'on': path, 'off': path}, compiled side by side where missing (about three minutes of host compile)."""
    todo = [w for w in FLAGS if not os.path.exists(lib_path(w))]
    if todo:
        os.makedirs(_native.BUILD, exist_ok=True)
        with ThreadPoolExecutor(len(todo)) as ex:
            list(ex.map(lambda w: _native.build_library([CFG], lib_path(w), f"fwdstream_{w}", jobs=1,
                                                        extra_flags=FLAGS[w]), todo))
    return {w: lib_path(w) for w in FLAGS}


if __name__ == "__main__":                               # what __graft_entry__.build() runs
    for _w, _p in build_libraries().items():
        print(_w, _p)
