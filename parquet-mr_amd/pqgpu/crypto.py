"""Parquet Modular Encryption, the part a page reader needs: the module AAD (AesCipher.createModuleAAD,
by pqg_module_aad) and the description of how one column chunk's pages are encrypted, which a
batch.ColumnChunk carries as `decryption` into Decoder.upload_chunks.

Keys are the caller's business (key retrieval and KMS are out of scope): a ColumnDecryption holds the
data key itself, as ModuleCipherFactory.getBlockDecryptor receives it."""
import ctypes as C

from . import abi, native

GCM, CTR = abi.DECRYPT_GCM, abi.DECRYPT_CTR
DATA_PAGE, DICTIONARY_PAGE = abi.MODULE_DATA_PAGE, abi.MODULE_DICTIONARY_PAGE


def module_aad(file_aad, module_type, row_group_ordinal, column_ordinal, page_ordinal=-1):
    """AesCipher.createModuleAAD for DATA_PAGE (with the page ordinal) and DICTIONARY_PAGE (without):
    file_aad || type || row group (2 bytes LE) || column (2 bytes LE) [|| page (2 bytes LE)].
    Raises PqgError(ERR_INVALID_ARG) for a negative ordinal, one above Short.MAX_VALUE or another type."""
    file_aad = bytes(file_aad)
    out = (C.c_uint8 * (len(file_aad) + 8))()
    n = C.c_uint32()
    src = (C.c_uint8 * max(len(file_aad), 1)).from_buffer_copy(file_aad or b"\0")
    rc = native.lib().pqg_module_aad(src, len(file_aad), int(module_type), int(row_group_ordinal), int(column_ordinal),
                                     int(page_ordinal), out, len(out), C.byref(n))
    native.check(rc, what="pqg_module_aad")
    return bytes(out[: n.value])


class ColumnDecryption:
    """How the pages of one column chunk are encrypted: the column's data key, the file AAD
    (InternalFileDecryptor.getFileAAD: aad_prefix || aad_file_unique), the chunk's row-group and column
    ordinals and the mode of its page modules (GCM for AES_GCM_V1, CTR for AES_GCM_CTR_V1)."""

    def __init__(self, key, file_aad, row_group_ordinal, column_ordinal, mode=GCM):
        self.key = bytes(key)
        self.file_aad = bytes(file_aad)
        self.row_group_ordinal = int(row_group_ordinal)
        self.column_ordinal = int(column_ordinal)
        self.mode = int(mode)
        if self.mode not in (GCM, CTR):
            raise native.PqgError(abi.ERR_INVALID_ARG, what=f"decryption mode {mode}")

    def overhead(self):
        """Bytes a module adds to its plaintext."""
        return abi.AES_SIZE_LENGTH + abi.AES_NONCE_LENGTH + (abi.AES_GCM_TAG_LENGTH if self.mode == GCM else 0)

    def page_aad(self, page_ordinal):
        return module_aad(self.file_aad, DATA_PAGE, self.row_group_ordinal, self.column_ordinal, page_ordinal)

    def dictionary_aad(self):
        return module_aad(self.file_aad, DICTIONARY_PAGE, self.row_group_ordinal, self.column_ordinal)
