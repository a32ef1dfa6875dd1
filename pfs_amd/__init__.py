"""pfs_amd — MI355X-native PFS chunk-ingest path (CDC rolling hash + BLAKE2b content hash).

Product modules: ``cdc`` (batch GPU API), ``chunk`` (chunk.Writer mirror), ``distributed``
(file sharding + RCCL gather of the chunk-ref index), ``fileset`` (filesets, their Sources and
the file RPCs over them).  Native code: ``libpfscdc.so`` (HIP kernels for gfx950 + C ABI in
``include/pfscdc.h``).
"""
from ._lib import INFO_CHILD, INFO_MATCH, SRC_GLOB  # noqa: F401
from .cdc import ChunkParams, Chunker, ScanResult, synthetic_bytes  # noqa: F401
from .fileset import glob_match  # noqa: F401

__all__ = ["ChunkParams", "Chunker", "ScanResult", "synthetic_bytes", "glob_match", "SRC_GLOB",
           "INFO_CHILD", "INFO_MATCH"]
