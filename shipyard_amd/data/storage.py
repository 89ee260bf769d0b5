"""Local object store — the Azure Blob/File analogue.

The reference stores resource files, global resources and task data in
Azure Storage containers (reference convoy/storage.py:68-88).  Here a
storage account is a directory root on the node's NVMe; containers are
subdirectories; blobs are files.  Upload/download optionally pack
through SYSHARD (LZ4 blocks + CRC32C manifest) so the GPU decode path
can consume them directly.
"""
from __future__ import annotations

import fnmatch
import shutil
from pathlib import Path
from typing import Iterator, List, Optional

from shipyard_amd.data import integrity, shardfmt


class ObjectStore:
    def __init__(self, root, create: bool = True):
        # resolve at init: list()/_path() compare against absolute
        # paths, so a relative root (cwd-dependent) must be pinned
        self.root = Path(root).resolve()
        if create:
            self.root.mkdir(parents=True, exist_ok=True)

    def _path(self, remote_path: str) -> Path:
        p = (self.root / remote_path.lstrip("/")).resolve()
        root = self.root.resolve()
        # containment check must be path-component aware: a raw string
        # prefix would let '../store-x/f' escape into a sibling whose
        # name shares the root's prefix.
        if p != root and root not in p.parents:
            raise ValueError(f"path escapes store root: {remote_path}")
        return p

    def exists(self, remote_path: str) -> bool:
        return self._path(remote_path).exists()

    def upload_bytes(self, remote_path: str, data: bytes,
                     pack: bool = False,
                     manifest: bool = False,
                     shuffle_elem: int = 0,
                     delta_elem: int = 0,
                     bitshuffle_elem: int = 0) -> Path:
        """``shuffle_elem`` (with ``pack``): byte-shuffle filter element
        size for typed numeric payloads; ``delta_elem``: delta filter
        element size for monotone ones (offsets, sorted ids,
        timestamps); ``bitshuffle_elem``: bit-shuffle filter element
        size for float weights and fields, in the byte shuffle's place.
        See shardfmt.pack."""
        dst = self._path(remote_path)
        dst.parent.mkdir(parents=True, exist_ok=True)
        if pack:
            dst = dst.with_suffix(dst.suffix + ".syshard")
            # GPU authoring when present (bit-identical output);
            # threaded CPU matcher otherwise
            workers = 0 if len(data) > (4 << 20) else None
            dst.write_bytes(shardfmt.pack_auto(
                data, workers=workers, shuffle_elem=shuffle_elem,
                delta_elem=delta_elem, bitshuffle_elem=bitshuffle_elem))
        else:
            dst.write_bytes(data)
        if manifest:
            integrity.write_manifest(dst, integrity.compute_cpu(data))
        return dst

    def upload_file(self, local_path, remote_path: str,
                    pack: bool = False, manifest: bool = False,
                    shuffle_elem: int = 0,
                    delta_elem: int = 0,
                    bitshuffle_elem: int = 0) -> Path:
        data = Path(local_path).read_bytes() if (pack or manifest) else None
        if pack or manifest:
            return self.upload_bytes(remote_path, data, pack=pack,
                                     manifest=manifest,
                                     shuffle_elem=shuffle_elem,
                                     delta_elem=delta_elem,
                                     bitshuffle_elem=bitshuffle_elem)
        dst = self._path(remote_path)
        dst.parent.mkdir(parents=True, exist_ok=True)
        shutil.copy2(local_path, dst)
        return dst

    def download_bytes(self, remote_path: str,
                       verify: bool = True, unpack: bool = True) -> bytes:
        p = self._path(remote_path)
        if not p.exists() and p.with_suffix(p.suffix + ".syshard").exists():
            p = p.with_suffix(p.suffix + ".syshard")
        data = p.read_bytes()
        if p.suffix == ".syshard" or data[:8] == shardfmt.MAGIC:
            if not unpack:
                return data  # raw SYSHARD: consumer decodes (GPU stager)
            return shardfmt.unpack_cpu(data, verify=verify)
        if verify:
            m = integrity.read_manifest(p)
            if m is not None:
                got = integrity.compute_cpu(data, m.chunk_size)
                if not integrity.verify(m, got):
                    raise ValueError(f"integrity failure: {remote_path}")
        return data

    def download_file(self, remote_path: str, local_path,
                      verify: bool = True) -> Path:
        data = self.download_bytes(remote_path, verify=verify)
        dst = Path(local_path)
        dst.parent.mkdir(parents=True, exist_ok=True)
        dst.write_bytes(data)
        return dst

    def delete(self, remote_path: str) -> bool:
        p = self._path(remote_path)
        if p.is_dir():
            shutil.rmtree(p)
            return True
        if p.exists():
            p.unlink()
            return True
        return False

    def list(self, prefix: str = "",
             include: Optional[List[str]] = None,
             exclude: Optional[List[str]] = None) -> Iterator[str]:
        base = self._path(prefix) if prefix else self.root
        if not base.exists():
            return
        for p in sorted(base.rglob("*")):
            if not p.is_file() or p.name.endswith(".manifest.json"):
                continue
            rel = p.relative_to(self.root).as_posix()
            name = p.relative_to(base).as_posix()
            if include and not any(fnmatch.fnmatch(name, pat)
                                   for pat in include):
                continue
            if exclude and any(fnmatch.fnmatch(name, pat)
                               for pat in exclude):
                continue
            yield rel
