"""Python mirror of the reference's vecfc.Index API over the HIP C ABI.

``lachesis-base_amd/build/liblachesis_hip.so`` (include/lachesis_hip.h) is
the product; this package is a thin ctypes layer used by tests and the bench,
shaped like the reference's Go API so the parity tests read like
vecfc/forkless_cause_test.go:

* :class:`Index`      -- dense-index handle (what a cgo shim binds 1:1)
* :class:`VecfcIndex` -- hash-keyed facade: ``reset(validators, get_event)``,
  ``add(e)``, ``flush()``, ``drop_not_flushed()``, ``forkless_cause(a, b)``,
  ``get_highest_before(id)``, ``dfs_subgraph``, ``branches_info`` ...
  (vecfc/index.go, vecfc/forkless_cause.go); ``new_index``,
  ``new_index_with_engine``, ``default_config``, ``lite_config`` as in
  vecfc/index.go:52-89
* :mod:`batcher`      -- level-synchronous DAG batcher (include/lachesis_batcher.h):
  parents-first buffering, bulk release in topological levels
* :mod:`emitter`      -- emitter/ancestor.QuorumIndexer over include/lachesis_emitter.h
* :mod:`mediantime`   -- vecmt's MedianTime / merged HighestBeforeTime over
  include/lachesis_mediantime.h (:class:`MedianTimeIndex`)
* :mod:`ancestry`     -- DfsSubgraph / confirmEvents as scans of the vector clock
  over include/lachesis_ancestry.h (:class:`AncestryIndex`), and fork
  evidence: the two events behind each cheater a head observes
* :mod:`abft`         -- abft.IndexedLachesis over include/lachesis_abft.h:
  frames, roots, election, blocks with batched ForklessCause on the GPU

There is no CPU fallback: importing this package on a machine without the
built library raises, and every compute call goes to the GPU.
"""

from .capi import Index, LxError, RowsegComm, ShardComm, load_library, shard_comm_unique_id  # noqa: F401
from .vecfc import (VecfcIndex, HighestBeforeSeq, LowestAfterSeq, BranchSeq, IndexConfig,  # noqa: F401
                    IndexCacheConfig, Ratio, default_config, lite_config, new_index, new_index_with_engine)
from . import tools  # noqa: F401
from . import abft  # noqa: F401
from . import emitter  # noqa: F401
from . import batcher  # noqa: F401
from . import mediantime  # noqa: F401
from .mediantime import MedianTimeIndex  # noqa: F401
from . import ancestry  # noqa: F401
from .ancestry import AncestryIndex  # noqa: F401
