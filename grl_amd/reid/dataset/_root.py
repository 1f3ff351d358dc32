"""Dataset root resolution and the presence check shared by the dataset classes."""
import os
import os.path as osp


def resolve_root(root, data_dir, env, subdir, marker):
    """Dataset root: ``root`` if given, else ``$env``, else ``data_dir`` itself when it holds ``marker``, else
    ``data_dir/subdir``.  The reference hard-codes its roots and ignores ``--data-dir`` for MARS and Duke."""
    if root:
        return root
    if os.environ.get(env):
        return os.environ[env]
    if not data_dir:
        raise RuntimeError("no dataset root: pass root=, set %s, or give a data_dir that holds '%s' or '%s/'"
                           % (env, marker, subdir))
    if osp.exists(osp.join(data_dir, marker)):
        return data_dir
    return osp.join(data_dir, subdir)


def check_paths(paths):
    """The reference's ``_check_before_run``: the first missing path raises RuntimeError naming it."""
    for p in paths:
        if not osp.exists(p):
            raise RuntimeError("'{}' is not available".format(p))
