"""KV-block offload data plane: GPU HBM -> pinned host DRAM -> filesystem.

Python layer over the native ``_kvoffload`` engine (HIP/CDNA4). Capability
parity with the reference ``kv_connectors/llmd_fs_backend``:

- ``file_mapper``   content-addressed storage layout
- ``engine``        torch -> native engine construction
- ``handlers``      transfer building (per-file splits, partial chunks)
- ``manager``       scheduler-side lookup / prepare / complete + events
- ``events``        storage-tier KVEvents publisher (feeds the indexer)

``OffloadEngineConfig(checksum=True)`` appends a 16-byte checksum footer to
every (block, layer) record and verifies each loaded span before a KV page
is written; ``record_checksum`` / ``tile_record_bytes`` describe the format
for tools (docs/architecture.md).
"""
from .engine import (  # noqa: F401
    CHECKSUM_DTYPE_SUFFIX,
    CHECKSUM_FOOTER_BYTES,
    CHECKSUM_MAGIC,
    OffloadEngineConfig,
    TorchOffloadEngine,
    record_checksum,
    tile_record_bytes,
)
from .file_mapper import FileMapper, KVCacheLayoutConfig  # noqa: F401
from .handlers import GPUToStorageHandler, StorageToGPUHandler, TransferResult  # noqa: F401
from .manager import SharedStorageOffloadManager  # noqa: F401
