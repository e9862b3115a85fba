"""phant_amd.types <-> the keccak256 users of src/types/ (receipt.zig logs bloom, transaction.zig hashes, block.zig headers)."""
from . import block, receipt, transaction  # noqa: F401
